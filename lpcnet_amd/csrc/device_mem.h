/*
 * device_mem.h -- who owns a batch's device memory: move-only owners of a
 * device buffer, a pinned host buffer, a stream and an event; DeviceTables,
 * the buffers of one upload list; Carver, one buffer carved into aligned
 * parts; and StateRows, the zero / save / restore of per-stream state.
 *
 * Everything here goes through the few free functions declared first, which
 * device_mem.cpp defines with HIP.  This header includes no HIP, and the seam
 * exists for one reason: tools/device_mem_check.cpp defines the same functions
 * with malloc and counters and checks the owners on the CPU.
 *
 * Invariant: an owner is released with its batch's device current.  The call
 * sites guarantee it: lpcnet_batch_destroy, lpcnet_batch_load_model, load_model
 * and pool_release set the device before anything is freed.
 */
#ifndef LPCNET_DEVICE_MEM_H
#define LPCNET_DEVICE_MEM_H

#include <stddef.h>
#include <string.h>

#include <utility>
#include <vector>

/* hipStream_t and hipEvent_t, as hip_runtime_api.h declares them */
struct ihipStream_t;
struct ihipEvent_t;

namespace lpcnet_mi355x {

using DevStreamHandle = ihipStream_t *;
using DevEventHandle = ihipEvent_t *;

/* ---- the backend (device_mem.cpp; a fake in tools/device_mem_check.cpp) ----
 * Allocations return null, the others -1, on failure (the HIP backend has
 * then set the thread's error).  dm_alloc_finegrained's memory is freed by
 * dm_free.  dm_upload and dm_download are blocking copies; dm_zero queues on
 * `s`, or blocks when s is null. */
void *dm_alloc(size_t bytes);
void *dm_alloc_finegrained(size_t bytes);
void dm_free(void *p);
void *dm_alloc_pinned(size_t bytes, bool mapped);
void dm_free_pinned(void *p);
int dm_upload(void *dst, const void *src, size_t bytes);
int dm_download(void *dst, const void *src, size_t bytes);
int dm_zero(void *dst, size_t bytes, DevStreamHandle s);
int dm_stream_sync(DevStreamHandle s);
DevStreamHandle dm_stream_create(); /* non-blocking */
void dm_stream_destroy(DevStreamHandle s);
DevEventHandle dm_event_create(bool timing);
void dm_event_destroy(DevEventHandle e);

/* ---- owners ---------------------------------------------------------------- */
/* One handle, released once: what the four owners below share.  Converts to
 * the handle, so code that reads b->d_state or b->stream stays as written. */
template <class H, void (*Release)(H)>
class Owner {
 protected:
  H h = nullptr;

 public:
  Owner() = default;
  Owner(Owner &&o) noexcept : h(o.h) { o.h = nullptr; }
  Owner &operator=(Owner &&o) noexcept
  {
    if (this != &o) {
      reset();
      h = o.h;
      o.h = nullptr;
    }
    return *this;
  }
  ~Owner() { reset(); }
  void reset()
  {
    if (h) Release(h);
    h = nullptr;
  }
  void swap(Owner &o) { std::swap(h, o.h); }
  operator H() const { return h; }
};

template <class T>
inline void dm_free_as(T *p) { dm_free((void *)p); }
template <class T>
inline void dm_free_pinned_as(T *p) { dm_free_pinned((void *)p); }

/* n elements of device memory; alloc releases what it held: 0 / -1 */
template <class T>
struct DevPtr : Owner<T *, dm_free_as<T>> {
  int alloc(size_t n)
  {
    this->reset();
    this->h = (T *)dm_alloc(n * sizeof(T));
    return this->h ? 0 : -1;
  }
  int alloc_finegrained(size_t n)
  {
    this->reset();
    this->h = (T *)dm_alloc_finegrained(n * sizeof(T));
    return this->h ? 0 : -1;
  }
};

/* n elements of pinned host memory, mapped into the device's address space or not */
template <class T>
struct PinnedPtr : Owner<T *, dm_free_pinned_as<T>> {
  int alloc(size_t n, bool mapped)
  {
    this->reset();
    this->h = (T *)dm_alloc_pinned(n * sizeof(T), mapped);
    return this->h ? 0 : -1;
  }
};

struct DevStream : Owner<DevStreamHandle, dm_stream_destroy> {
  int create()
  {
    reset();
    h = dm_stream_create();
    return h ? 0 : -1;
  }
};

struct DevEvent : Owner<DevEventHandle, dm_event_destroy> {
  int create(bool timing)
  {
    reset();
    h = dm_event_create(timing);
    return h ? 0 : -1;
  }
};

/* The timing events of a batch (mark, lpcnet_batch_reset_timers): raw handles,
 * handed out (taken) or waiting for reuse (idle), all destroyed here. */
struct EventPool {
  std::vector<DevEventHandle> taken, idle;
  EventPool() = default;
  EventPool(const EventPool &) = delete;
  EventPool &operator=(const EventPool &) = delete;
  ~EventPool()
  {
    for (DevEventHandle e : taken) dm_event_destroy(e);
    for (DevEventHandle e : idle) dm_event_destroy(e);
  }
  /* an idle event, or a new one; it is `taken` from here on (null: none to be had) */
  DevEventHandle take()
  {
    DevEventHandle e = nullptr;
    if (!idle.empty()) {
      e = idle.back();
      idle.pop_back();
    } else {
      e = dm_event_create(true);
    }
    if (e) taken.push_back(e);
    return e;
  }
  void recycle()
  {
    idle.insert(idle.end(), taken.begin(), taken.end());
    taken.clear();
  }
};

/* ---- the buffers of an upload list ----------------------------------------- */
/* one table of a model: its host bytes and where its device address goes */
struct ModelUpload {
  void *dst; /* address of a pointer member of the kernels' arguments */
  const void *src;
  size_t bytes;
  bool present;
};

class DeviceTables {
  std::vector<DevPtr<char>> bufs;

 public:
  /* One buffer per present entry, in list order (16 bytes for an empty
   * entry), its contents copied and its address stored through dst.  On any
   * failure: frees what this call allocated, keeps what the object held, -1. */
  int upload(const std::vector<ModelUpload> &up)
  {
    const size_t held = bufs.size();
    for (const ModelUpload &u : up) {
      if (!u.present) continue;
      DevPtr<char> p;
      if (p.alloc(u.bytes ? u.bytes : 16) || (u.bytes && dm_upload(p, u.src, u.bytes))) {
        bufs.resize(held);
        return -1;
      }
      char *a = p;
      memcpy(u.dst, &a, sizeof(a));
      bufs.push_back(std::move(p));
    }
    return 0;
  }
  /* a zeroed buffer of its own (null on failure, nothing kept) */
  void *zeroed(size_t bytes)
  {
    DevPtr<char> p;
    if (p.alloc(bytes) || dm_zero(p, bytes, nullptr)) return nullptr;
    bufs.push_back(std::move(p));
    return bufs.back();
  }
  void clear() { bufs.clear(); }
  void swap(DeviceTables &o) { bufs.swap(o.bufs); }
  size_t size() const { return bufs.size(); }
};

/* ---- one allocation carved into parts --------------------------------------- */
/* add(p, n) plans n elements behind the pointer p, 256-byte aligned; alloc()
 * allocates the whole, sets every planned pointer and returns the owner of
 * the base (empty, the pointers untouched, when the device refuses). */
class Carver {
  struct Part {
    void *ptr; /* the T * to set */
    size_t off;
  };
  std::vector<Part> parts;
  size_t bytes = 0;

 public:
  template <class T>
  void add(T *&p, size_t n)
  {
    parts.push_back({&p, bytes});
    bytes += (n * sizeof(T) + 255) & ~(size_t)255;
  }
  size_t size() const { return bytes; }
  DevPtr<char> alloc()
  {
    DevPtr<char> base;
    if (base.alloc(bytes)) return base;
    for (const Part &q : parts) {
      char *p = base + q.off;
      memcpy(q.ptr, &p, sizeof(p));
    }
    return base;
  }
};

/* ---- per-stream state rows --------------------------------------------------- */
/* rows of `bytes` bytes per stream at `base`: stream s owns [s bytes, (s + 1) bytes) */
struct StateRows {
  void *base;
  size_t bytes;
  char *row(size_t s) const { return (char *)base + s * bytes; }
};

/* queue on q the zeroing of one stream's rows, or of all B (stream < 0) */
inline int rows_zero(const std::vector<StateRows> &rows, int stream, int B, DevStreamHandle q)
{
  const size_t first = stream < 0 ? 0 : (size_t)stream, n = stream < 0 ? (size_t)B : 1;
  for (const StateRows &r : rows)
    if (dm_zero(r.row(first), n * r.bytes, q)) return -1;
  return 0;
}

/* one stream's rows into buf, back to back, after everything queued on q */
inline int rows_save(const std::vector<StateRows> &rows, int stream, void *buf, DevStreamHandle q)
{
  if (dm_stream_sync(q)) return -1;
  char *out = (char *)buf;
  for (const StateRows &r : rows) {
    if (dm_download(out, r.row((size_t)stream), r.bytes)) return -1;
    out += r.bytes;
  }
  return 0;
}

inline int rows_restore(const std::vector<StateRows> &rows, int stream, const void *buf, DevStreamHandle q)
{
  if (dm_stream_sync(q)) return -1;
  const char *in = (const char *)buf;
  for (const StateRows &r : rows) {
    if (dm_upload(r.row((size_t)stream), in, r.bytes)) return -1;
    in += r.bytes;
  }
  return 0;
}

}  // namespace lpcnet_mi355x

#endif
