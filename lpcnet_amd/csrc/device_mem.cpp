/*
 * device_mem.cpp -- device_mem.h's backend on HIP: the one place the library
 * allocates and frees device and pinned memory, streams and events (the
 * public allocator lpcnet_batch_device_alloc / _free of engine.cpp aside).
 * A call that fails sets the thread's error to HIP's.
 */
#include <hip/hip_runtime.h>

#include <string>

#include "device_mem.h"
#include "model_host.h"

namespace lpcnet_mi355x {

static int chk(hipError_t e, const char *what)
{
  if (e == hipSuccess) return 0;
  set_err(std::string(what) + ": " + hipGetErrorString(e));
  return -1;
}

void *dm_alloc(size_t bytes)
{
  void *p = nullptr;
  return chk(hipMalloc(&p, bytes), "hipMalloc") ? nullptr : p;
}

void *dm_alloc_finegrained(size_t bytes)
{
  void *p = nullptr;
  return chk(hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained), "hipExtMallocWithFlags") ? nullptr : p;
}

void dm_free(void *p) { (void)hipFree(p); }

void *dm_alloc_pinned(size_t bytes, bool mapped)
{
  void *p = nullptr;
  return chk(hipHostMalloc(&p, bytes, mapped ? hipHostMallocMapped : hipHostMallocDefault), "hipHostMalloc") ? nullptr : p;
}

void dm_free_pinned(void *p) { (void)hipHostFree(p); }

int dm_upload(void *dst, const void *src, size_t bytes) { return chk(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice), "hipMemcpy"); }

int dm_download(void *dst, const void *src, size_t bytes) { return chk(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost), "hipMemcpy"); }

int dm_zero(void *dst, size_t bytes, hipStream_t s)
{
  return s ? chk(hipMemsetAsync(dst, 0, bytes, s), "hipMemsetAsync") : chk(hipMemset(dst, 0, bytes), "hipMemset");
}

int dm_stream_sync(hipStream_t s) { return chk(hipStreamSynchronize(s), "hipStreamSynchronize"); }

hipStream_t dm_stream_create()
{
  hipStream_t s = nullptr;
  return chk(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), "hipStreamCreateWithFlags") ? nullptr : s;
}

void dm_stream_destroy(hipStream_t s) { (void)hipStreamDestroy(s); }

hipEvent_t dm_event_create(bool timing)
{
  hipEvent_t e = nullptr;
  const hipError_t rc = timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming);
  return chk(rc, "hipEventCreate") ? nullptr : e;
}

void dm_event_destroy(hipEvent_t e) { (void)hipEventDestroy(e); }

}  // namespace lpcnet_mi355x
