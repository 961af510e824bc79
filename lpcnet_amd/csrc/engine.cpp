/*
 * engine.cpp -- host side of the MI355X LPCNet synthesis engine and the
 * batch entry points (lpcnet_batch_*, model checks) declared in
 * include/lpcnet_mi355x.h.  The drop-in single-stream API of include/lpcnet.h
 * is dropin.cpp, over the partial-batch steps declared in batch.h.  The calls
 * beside synthesis -- the PLC predictor, the feature extractor and
 * lpcnet_mi355x_device_lpc -- are side_calls.cpp, their host-built tables
 * side_tables.cpp (host-only); this file loads and frees the PLC tables with
 * the model (plc_load, plc_free) and lends them its timed regions (batch.h).
 *
 * Responsibilities
 *  - upload of a parsed, validated and re-tiled weight blob (model_host.cpp:
 *    blob -> HostModel; mf_plan.cpp: the GRU_A planner and register tables
 *    of the matrix-core kernels; both host-only) and its commit to a batch;
 *  - per-stream device state (lpcnet_private.h:28-48) and reset semantics
 *    (lpcnet.c:174-182);
 *  - per-frame scheduling: lpc_kernel (lpc_from_cepstrum), frame_kernel and
 *    the sample kernel on the batch's HIP stream (the first two on a second
 *    stream, one frame ahead, for small batches).  Which sample kernel and
 *    which frame path a call takes is decided in kernel_choice.cpp
 *    (host-only): this file fills its arguments and acts on the answer.
 * Compile with -ffp-contract=off, as every translation unit.
 */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cstddef>
#include <chrono>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "batch.h"

namespace {

/* kiss99.c:32-81 */
struct Kiss {
  uint32_t z, w, jsr, jcong;
  uint32_t next()
  {
    uint32_t znew = 36969 * (z & 0xFFFF) + (z >> 16);
    uint32_t wnew = 18000 * (w & 0xFFFF) + (w >> 16);
    uint32_t mwc = (znew << 16) + wnew;
    uint32_t shr3 = jsr ^ (jsr << 13);
    shr3 ^= shr3 >> 17;
    shr3 ^= shr3 << 5;
    uint32_t cong = 69069 * jcong + 1234567;
    z = znew; w = wnew; jsr = shr3; jcong = cong;
    return (mwc ^ cong) + shr3;
  }
  void srand(const unsigned char *d, int n)
  {
    int i;
    z = 362436069; w = 521288629; jsr = 123456789; jcong = 380116160;
    for (i = 3; i < n; i += 4) {
      z ^= d[i - 3]; w ^= d[i - 2]; jsr ^= d[i - 1]; jcong ^= d[i];
      next();
    }
    if (i - 3 < n) z ^= d[i - 3];
    if (i - 2 < n) w ^= d[i - 2];
    if (i - 1 < n) jsr ^= d[i - 1];
    if (z == 0 || z == 0x9068FFFF) z++;
    if (w == 0 || w == 0x464FFFFF) w++;
    if (jsr == 0) jsr++;
  }
};

}  // namespace

/* ---- launcher helpers (lpcnet_engine.h), keyed by the current device ---- */
namespace lpcnet_mi355x {

int ensure_dyn_lds(const void *kernel, int bytes)
{
  static std::mutex mu;
  static std::map<std::pair<const void *, int>, int> done; /* (kernel, device) -> bytes set */
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return -1;
  std::lock_guard<std::mutex> lk(mu);
  int &have = done[{kernel, dev}];
  if (have >= bytes) return 0;
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return -1;
  have = bytes;
  return 0;
}

int current_device_cus()
{
  static std::mutex mu;
  static std::map<int, int> cus;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cus.find(dev);
  if (it != cus.end()) return it->second;
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
  cus[dev] = n;
  return n;
}

}  // namespace lpcnet_mi355x

namespace {

void free_model(LPCNetBatch *b)
{
  for (void *p : b->model_bufs) (void)hipFree(p);
  b->model_bufs.clear();
  b->have_model = false;
  b->ck_warm = L2Warm{};
}

hipEvent_t get_event(LPCNetBatch *b)
{
  if (!b->ev_free.empty()) {
    hipEvent_t e = b->ev_free.back();
    b->ev_free.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

/* what the kernel choice (kernel_choice.cpp) takes from a host model, and
 * the kernels' dynamic LDS for it */
ModelCaps model_caps(const HostModel &h)
{
  ModelCaps c;
  c.fp_ok = h.fp_ok;
  c.mf_ok = h.mf_ok;
  c.mf_split = h.sa.mf_split != 0;
  c.mfw_split = h.sa.mfw_split != 0;
  c.reg = h.reg;
  c.S = h.S;
  c.lds_bytes = h.lds;
  c.mf_ga_ops = h.mf_ga_ops;
  c.mf_gb_ops = h.mf_gb_ops;
  return c;
}

LdsSizes lds_sizes(const ModelCaps &c)
{
  LdsSizes l;
  l.fp = fp_lds_bytes();
  l.mf = mf_lds_bytes(c.S, c.mf_split);
  l.mf2 = mf2_lds_bytes(c.mf_split);
  l.mfw[0] = mfw_lds_bytes(2, c.mf_split);
  l.mfw[1] = mfw_lds_bytes(3, c.mf_split);
  return l;
}

/* whether a batch like this will run mfw_kernel, under the environment as it
 * is now: the plan class its register tables are built for */
bool wide_now(int B, int kernel_mode, bool rcp_custom, int cus)
{
  return plans_wide(B, kernel_mode, rcp_custom, cus, choice_env_from_env());
}

/* the batch's plan and the info fields that follow it, after a load or a
 * change of the kernel mode or the rcpps table */
void plan_batch(LPCNetBatch *b)
{
  b->plan = plan_sample_kernels(b->caps, lds_sizes(b->caps), b->B, current_device_cus(), b->kernel_mode, b->rcp_custom,
                                choice_env_from_env());
  b->sa.rcp_hw = b->fa.rcp_hw = b->plan.rcp_hw;
  b->info.rcp_hw = b->plan.rcp_hw;
  b->info.quad_path = b->plan.quad_path;
  b->info.streams_per_workgroup = b->plan.streams_per_workgroup;
  b->info.lds_bytes = b->plan.lds_bytes;
  b->info.mfma_ops_per_group_sample = b->plan.mfma_ops_per_group_sample;
}

/* what a model build takes from the batch size and the kernels */
ModelBuildOpts build_opts(int streams, bool wide)
{
  ModelBuildOpts o;
  o.streams = streams;
  o.wide = wide;
  for (int v = 0; v < 2; v++)
    for (int k = 0; k < 3; k++) o.lds_extra[v][k] = sample_lds_bytes(1 << k, v, 0);
  return o;
}

/* One device buffer per entry of the model's upload list, its address in
 * the entry's member of `args`.  On any failure frees what it allocated. */
int upload_model(const HostModel &host, ModelArgs &args, std::vector<void *> &bufs)
{
  const std::vector<ModelUpload> up = model_uploads(host, args);
  for (const ModelUpload &u : up) {
    if (!u.present) continue;
    void *p = nullptr;
    bool ok = hipMalloc(&p, u.bytes ? u.bytes : 16) == hipSuccess;
    if (ok) bufs.push_back(p);
    ok = ok && (!u.bytes || hipMemcpy(p, u.src, u.bytes, hipMemcpyHostToDevice) == hipSuccess);
    if (!ok) {
      for (void *q : bufs) (void)hipFree(q);
      bufs.clear();
      set_err("device upload failed");
      return -1;
    }
    memcpy(u.dst, &p, sizeof(p));
  }
  return 0;
}

/* Parse, validate and re-tile a weight blob into `host` (model_host.cpp),
 * upload it and make it the batch's model.  A fresh load frees the previous
 * model's buffers before it uploads, so a failed upload leaves no model at
 * all (have_model false); a failed build leaves the previous model intact.
 * replan: the batch's own blob again, for new register tables only
 * (replan_if_needed): the new tables are uploaded beside the old ones, which
 * are freed only once the new ones stand. */
int load_model(LPCNetBatch *b, const unsigned char *data, int len, HostModel &host, bool replan = false)
{
  ModelBuildOpts opts = build_opts(b->B, wide_now(b->B, b->kernel_mode, b->rcp_custom, current_device_cus()));
  opts.replan = replan;
  opts.mc = b->mc;
  opts.rcp_custom = b->rcp_custom;
  opts.rcp_dev = (int)b->rcp_dev.size() == RCP_ENTRIES ? b->rcp_dev.data() : nullptr;
  if (build_host_model(data, len, opts, host)) return -1;
  if (b->set_device()) { set_err("hipSetDevice failed"); return -1; }
  if (!replan) free_model(b);
  ModelArgs args;
  std::vector<void *> bufs;
  if (upload_model(host, args, bufs)) return -1;
  if (!host.bounds_note.empty()) fputs(host.bounds_note.c_str(), stderr);
  /* Nothing in *b (a fresh load's freed buffers aside) has changed up to
   * here, and nothing below can fail: every check passed and the last upload
   * succeeded. */
  for (void *p : b->model_bufs) (void)hipFree(p); /* a replan's previous tables */
  b->model_bufs = bufs;
  b->sa = args.sa;
  b->fa = args.fa;
  b->da = args.da;
  b->has_codebooks = host.cb_ok;
  b->mc = host.mc;
  b->rcp_custom = host.rcp_custom;
  b->rcp_dev = host.rcp_dev;
  b->variant = host.variant;
  b->sat = host.sat;
  b->caps = model_caps(host);
  b->plan_wide = host.plan_wide;
  b->image_bytes = (int)host.img.size();
  /* the chunk kernel's weights, one copy of each (deferred LPC warms them) */
  const float4 *wm[5] = {args.fa.ck_conv1, args.fa.ck_conv2, args.fa.ck_dense1, args.fa.ck_dense2, args.fa.ck_proj};
  for (int t = 0; t < 5; t++) {
    b->ck_warm.m[t] = (const uint32_t *)wm[t];
    b->ck_warm.lines[t] = (int)((t < 4 ? (size_t)host.ck_rep[t] * 4 : host.ck_proj.size()) * 4 / 128);
  }
  b->info = host.info;
  b->have_model = true;
  plan_batch(b); /* the rest of info, mfma_ops_per_group_sample for the chosen kernel */
  return 0;
}

int ensure_trace(LPCNetBatch *b, int N)
{
  if (!b->trace) {
    b->sa.trace_logits = nullptr;
    b->sa.trace_exc = nullptr;
    return 0;
  }
  if (!b->d_trace_logits) {
    HIPCHK(hipMalloc(&b->d_trace_logits, (size_t)b->B * FRAME * 8 * 4));
    HIPCHK(hipMalloc(&b->d_trace_exc, (size_t)b->B * FRAME * 4));
  }
  b->sa.trace_logits = b->d_trace_logits;
  b->sa.trace_exc = b->d_trace_exc;
  b->trace_N = N;
  return 0;
}

}  // namespace

/* ---- timed regions (lpcnet_batch_kernel_ms; batch.h) ---------------------- */
/* mark: with `on`, take an event and record it on `s` (e = nullptr
 * otherwise: with timing off there are no events at all).  The event belongs
 * to ev_taken from the moment it is taken, so a failing call leaks nothing.
 * timed: the pair (e0, e1) covers `frames` frames of region `which` (0 sample
 * kernel, 1 frame kernel, 2 PLC predictor, 3 feature extractor, 4 and 5 the
 * encoder, 6 the Burg analysis). */
int lpcnet_mi355x::mark(LPCNetBatch *b, bool on, hipStream_t s, hipEvent_t &e)
{
  e = nullptr;
  if (!on) return 0;
  e = get_event(b);
  if (!e) { set_err("hipEventCreate failed"); return -1; }
  b->ev_taken.push_back(e);
  HIPCHK(hipEventRecord(e, s));
  return 0;
}

void lpcnet_mi355x::timed(LPCNetBatch *b, int which, hipEvent_t e0, hipEvent_t e1, int frames)
{
  if (!e0 || !e1) return;
  b->ev_pairs[which].push_back(e0);
  b->ev_pairs[which].push_back(e1);
  b->ev_frames[which].push_back(frames);
}

namespace {

/* ---- the sample kernel of a launch ---------------------------------------- */
/* What every sample launch takes from the batch: N samples for its first nB
 * streams.  Callers set cond, nframes, pcm, preload and stamps. */
SampleArgs sample_args(const LPCNetBatch *b, int nB, int N)
{
  SampleArgs sa = b->sa;
  sa.st = b->d_state;
  sa.delay = b->mc.delay;
  sa.nstreams = nB;
  sa.N = N;
  sa.preload = 0;
  sa.stamps = nullptr;
  sa.status = b->d_status;
  sa.spin_limit = b->spin_limit;
  return sa;
}

/* the kernel a launch of the batch's first nB streams runs (the trace is the
 * batch's: ensure_trace) */
SampleKernel launch_kernel(const LPCNetBatch *b, int nB, bool preload, bool stamps)
{
  return kernel_for_launch(b->plan, nB, preload, b->sa.trace_logits != nullptr, stamps);
}

int launch_sample_kernel(LPCNetBatch *b, const SampleArgs &sa)
{
  if (sa.N <= 0) return 0;
  int rc = -1;
  switch (launch_kernel(b, sa.nstreams, sa.preload != 0, sa.stamps != nullptr)) {
  case SampleKernel::FP: rc = launch_fp(sa, b->stream); break;
  case SampleKernel::MFW: rc = launch_mfw(sa, b->plan.mfw_g, b->stream); break;
  case SampleKernel::MF2: rc = launch_mf2(sa, b->stream); break;
  case SampleKernel::MF: rc = launch_mf(sa, b->caps.S, mf_lds_bytes(b->caps.S, b->sa.mf_split), b->stream); break;
  case SampleKernel::LOCKSTEP:
    rc = launch_sample(sa, b->caps.S, b->variant, b->sat ? 1 : 0, b->caps.reg ? 1 : 0, b->caps.lds_bytes, b->stream);
    break;
  }
  if (rc) {
    set_err(std::string("sample kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
    return -1;
  }
  return 0;
}

/* ovl >= 0: overlapped form, frame f = ovl.  The frame kernel runs on
 * fstream, followed by a copy of its outputs into d_cond[f & 1] (which
 * sample kernel f-2 read: ev_samp); the sample kernel on stream waits only
 * for that copy (ev_frame) and reads the frame's outputs there, so frame
 * kernel f+1 runs beside sample kernel f.  The sample kernels read nothing
 * else the frame kernel writes.  Every fstream launch precedes a stream
 * launch that waits for it, so a sync of stream covers both. */
/* d_lpc_frame: this frame's lpc_from_cepstrum output ([B][NLPC]); with
 * run_lpc the LPC kernel computing it is launched first, otherwise it was
 * computed earlier on the same queue (lpcnet_batch_synthesize_frames
 * batches it over many frames). */
int launch_frame_step(LPCNetBatch *b, const float *d_features, float *d_lpc_frame, bool run_lpc, short *d_pcm, int N,
                      int preload = 0, int ovl = -1, int nB = -1, bool run_frame = true, bool keep_cond = false)
{
  /* run_frame false: the sample network only, on the conditioning already in
   * the stream states (lpcnet_synthesize_tail_impl, lpcnet.c:235-271);
   * keep_cond: the frame network of run_frame_network_flush (lpcnet.c:134-144) */
  /* nB: run the first nB streams of the batch only (the drop-in pool's work
   * batch); the overlapped form always runs all of them */
  if (nB < 0 || ovl >= 0) nB = b->B;
  const int c = ovl & 1;
  hipStream_t fs = ovl >= 0 ? b->fstream : b->stream;
  FrameArgs fa = b->fa;
  fa.st = b->d_state;
  fa.mc = b->mc;
  fa.nstreams = nB;
  fa.features = d_features;
  fa.lpc_new = d_lpc_frame;
  fa.keep_cond = keep_cond ? 1 : 0;
  SampleArgs sa = sample_args(b, nB, N);
  sa.pcm = d_pcm;
  sa.preload = std::max(0, std::min(preload, N));
  sa.stamps = b->d_stamps;
  fa.stamps = b->d_stamps ? b->d_stamps + (size_t)b->B * STAMP_WAVES * 16 : nullptr;
  if (ovl >= 0) {
    sa.cond = b->d_cond[c];
  }
  /* timing 1: events around the sample kernel only; 2: the frame kernel too
   * (one event between the two kernels serves both pairs; the overlapped
   * form ends the frame kernel's pair on its own queue: ef) */
  hipEvent_t e0, ef = nullptr, e1, e2;
  if (ovl >= 0 && b->ev_samp_used[c]) HIPCHK(hipStreamWaitEvent(fs, b->ev_samp_cur[c], 0));
  if (mark(b, b->timing >= 2, fs, e0)) return -1;
  /* lpc_from_cepstrum of this frame's features: the frame kernel pushes it
   * into the two-frame LPC ring (lpcnet.c:110-112) */
  if (run_frame && run_lpc && !b->mc.end2end && launch_lpc(d_features, d_lpc_frame, nB, b->d_lpc_tab, fs)) {
    set_err("lpc kernel launch failed");
    return -1;
  }
  if (run_frame && launch_frame(fa, fs)) { set_err("frame kernel launch failed"); return -1; }
  if (ovl >= 0 && launch_cond_copy(b->d_state, b->d_cond[c], b->B, fs)) {
    set_err("copy launch failed");
    return -1;
  }
  if (ovl >= 0) {
    if (mark(b, e0 != nullptr, fs, ef)) return -1;
    /* an event, not a device flag: a sample kernel polling a flag set by
     * the other queue was faster by ~1 % but gave wrong output wherever the
     * two queues do not run concurrently (rocprofv3 --pmc serialises
     * dispatches: the poll timed out and read a stale slot) */
    HIPCHK(hipEventRecord(b->ev_frame[c], fs));
    HIPCHK(hipStreamWaitEvent(b->stream, b->ev_frame[c], 0));
  }
  if (mark(b, b->timing >= 1, b->stream, e1)) return -1;
  if (launch_sample_kernel(b, sa)) return -1;
  if (mark(b, b->timing >= 1, b->stream, e2)) return -1;
  if (ovl >= 0) {
    /* every event record is a queue packet (~5 us between two kernels at
     * batch 1): the timing event after the sample kernel serves as ev_samp */
    if (e2) {
      b->ev_samp_cur[c] = e2; /* recycled only by reset_timers, which clears the use */
    } else {
      HIPCHK(hipEventRecord(b->ev_samp[c], b->stream));
      b->ev_samp_cur[c] = b->ev_samp[c];
    }
    b->ev_samp_used[c] = true;
  }
  timed(b, 1, e0, ef ? ef : e1, 1);
  timed(b, 0, e1, e2, 1);
  if (run_frame) b->frames_done(1);
  return 0;
}

/* Chunked form: the frame network of frames [0, n) of d_features has run
 * (chunk_kernel, outputs in d_chunk[f]); launch the sample kernel of frames
 * f .. f + nfr - 1 on b->stream, reading their conditioning from d_chunk[f..]
 * and writing d_pcm [nfr][B][N].  nfr > 1: matrix-core kernel only, every
 * stream past its first `delay` frames (SampleArgs::nframes). */
int launch_chunk_samples(LPCNetBatch *b, int f, short *d_pcm, int N, int nfr = 1)
{
  SampleArgs sa = sample_args(b, b->B, N);
  sa.cond = b->d_chunk + (size_t)f * b->B;
  sa.nframes = nfr;
  sa.pcm = d_pcm;
  sa.stamps = b->d_stamps;
  return timed_launch(b, 0, b->timing >= 1, nfr, nullptr, [&] { return launch_sample_kernel(b, sa); });
}

/* Chunked form: the frame network of n frames (features [n][B][NF], their
 * LPC already in d_lpc) in one launch on b->stream. */
int launch_chunk_frames(LPCNetBatch *b, const float *d_features, int n)
{
  FrameArgs fa = b->fa;
  fa.st = b->d_state;
  fa.mc = b->mc;
  fa.nstreams = b->B;
  fa.features = d_features;
  fa.lpc_new = b->d_lpc;
  fa.nframes = n;
  fa.cond = b->d_chunk;
  fa.stamps = nullptr;
  if (timed_launch(b, 1, b->timing >= 2, n, "chunk kernel launch failed", [&] { return launch_chunk(fa, b->stream); })) return -1;
  b->frames_done(n);
  return 0;
}

/* After a sync of b->stream: report (and clear) a device-side abort. */
int check_status(LPCNetBatch *b)
{
  const int st = __atomic_load_n(b->h_status, __ATOMIC_ACQUIRE);
  if (st == 0) return 0;
  __atomic_store_n(b->h_status, 0, __ATOMIC_RELEASE);
  if (st & STATUS_FLAG_TIMEOUT)
    set_err("device abort: an LDS flag wait in the sample kernel exceeded its spin limit; the PCM of this call is invalid");
  else if (st & STATUS_SLICE_TIMEOUT)
    set_err("device abort: a sliced one-frame chunk kernel waited too long for its sibling workgroups; the PCM of "
            "this call is invalid");
  else if (st & STATUS_ACTIVITY)
    set_err("device abort: a multi-frame sample launch saw a stream turn active mid-launch (frame_count bound out of "
            "date); the PCM of this call is invalid");
  else
    set_err("device abort: unknown status " + std::to_string(st));
  return -1;
}

}  // namespace

/* ---- stream-state helpers (batch.h), host-only --------------------------- */
namespace lpcnet_mi355x {

void host_reset_state(StreamState &s)
{
  memset(&s, 0, sizeof(s));
  s.last_exc = host_lin2ulaw(0.f);
  Kiss k;
  k.srand((const unsigned char *)"LPCNet", 6);
  s.rng[0] = k.z; s.rng[1] = k.w; s.rng[2] = k.jsr; s.rng[3] = k.jcong;
}

/* lpcnet.c:226-233 lpcnet_reset_signal on one stream */
void reset_signal(StreamState &s)
{
  s.deemph_mem = 0;
  s.last_exc = host_lin2ulaw(0.f);
  memset(s.last_sig, 0, sizeof(s.last_sig));
  memset(s.gru_a_state, 0, sizeof(s.gru_a_state));
  memset(s.gru_b_state, 0, sizeof(s.gru_b_state));
}

/* GRU states are convex combinations of earlier states and tanh outputs:
 * |x| <= 1 (+ rounding) or NaN for every state the recurrence produces.
 * The int8 kernels' state quantiser relies on |x| < 2^24 (quant_s8_state),
 * so a snapshot outside that range is not one of ours: its restore refuses it. */
bool gru_state_plausible(const float *v, size_t n)
{
  for (size_t k = 0; k < n; k++)
    if (v[k] > 2.f || v[k] < -2.f) return false;
  return true;
}

/* A snapshot is restored only if it is one this engine can have produced. */
bool snapshot_ok(const void *buf)
{
  StreamState tmp;
  memcpy(&tmp, buf, sizeof(tmp));
  if (!gru_state_plausible(tmp.gru_a_state, NA) || !gru_state_plausible(tmp.gru_b_state, NB)) {
    set_err("snapshot GRU state outside [-2, 2]: not a state this engine produced");
    return false;
  }
  /* last_exc indexes the 256-row embedding tables (lpcnet.c:264: an
   * excitation is a u-law byte) */
  if (tmp.last_exc < 0 || tmp.last_exc > 255) {
    set_err("snapshot last_exc outside [0, 255]: not a state this engine produced");
    return false;
  }
  return true;
}

}  // namespace lpcnet_mi355x

/* ======================================================================== */
/* batch API                                                                 */

extern "C" {

LPCNET_EXPORT const char *lpcnet_mi355x_last_error(void) { return last_err().c_str(); }

/* Host-only view of the GRU_A plans a blob gets on a wide batch (no
 * device): the main plan (mf_plan, wide class) and, for split models, the
 * wide kernel's split tables.  out[0] = split (0/1), out[1] = mfw split form
 * available (0/1), out[2..17] = the split form's z/r and h 4-slot groups per
 * table wave (R waves 0..5, host waves 6..7), out[18..20] = pieces per gate.
 * 0 / -1 (malformed blob or no int8 matrix-core plan). */
LPCNET_EXPORT int lpcnet_mi355x_wide_plan(const unsigned char *data, int len, int *out)
{
  std::vector<Arr> L;
  if (!data || len <= 0 || !out || !parse_blob(L, data, len)) return -1;
  GruASparse A;
  if (parse_gru_a(L, A) || A.variant != LPCNET_VARIANT_INT8) return -1;
  const std::vector<std::vector<int>> &ga = A.blocks;
  const MfPlanParams pp = mf_plan_params_from_env();
  MfPlan plan;
  if (!mf_plan(ga, plan, pp, 3, 2)) return -1;
  MfwSplitTab T;
  const bool ok = plan.split && mfw_split_tables(ga, A.first, (const int8_t *)A.w, pp, T);
  out[0] = plan.split ? 1 : 0;
  out[1] = ok ? 1 : 0;
  for (int w = 0; w < MFW_TAB_WAVES; w++) {
    out[2 + 2 * w] = T.nzr[w];
    out[3 + 2 * w] = T.nh[w];
  }
  for (int g = 0; g < 3; g++) {
    int n = 0;
    for (int u = 0; u < NA / 8; u++) {
      const int K = (int)ga[g * (NA / 8) + u].size(), c = g < 2 ? MF_ZMAX : MF_HMAX;
      if (K > c) n += (K - c + c - 1) / c;
    }
    out[18 + g] = n;
  }
  return 0;
}

LPCNET_EXPORT int lpcnet_mi355x_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

LPCNET_EXPORT const uint32_t *lpcnet_mi355x_rcp_table(void) { return kRcpTable; }

LPCNET_EXPORT LPCNetBatch *lpcnet_batch_create(int nb_streams, int device)
{
  if (nb_streams < 1) { set_err("nb_streams < 1"); return nullptr; }
  int ndev = lpcnet_mi355x_device_count();
  if (device < 0 || device >= ndev) { set_err("no such HIP device"); return nullptr; }
  LPCNetBatch *b = new LPCNetBatch();
  b->device = device;
  b->B = nb_streams;
  bool ok = b->set_device() == 0;
  ok = ok && hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) == hipSuccess;
  ok = ok && hipMalloc(&b->d_state, sizeof(StreamState) * (size_t)nb_streams) == hipSuccess;
  ok = ok && hipMalloc(&b->d_feat, sizeof(float) * NF * (size_t)nb_streams) == hipSuccess;
  ok = ok && hipMalloc(&b->d_pcm, sizeof(short) * FRAME * (size_t)nb_streams) == hipSuccess;
  ok = ok && hipHostMalloc(&b->h_status, 64, hipHostMallocMapped) == hipSuccess;
  ok = ok && hipHostGetDevicePointer((void **)&b->d_status, b->h_status, 0) == hipSuccess;
  if (ok) *b->h_status = 0;
  ok = ok && hipMalloc(&b->d_lpc, sizeof(float) * NLPC * (size_t)nb_streams * LPC_CHUNK) == hipSuccess;
  ok = ok && hipMalloc(&b->d_ck_sync, sizeof(int) * (size_t)((nb_streams + 15) / 16)) == hipSuccess;
  ok = ok && hipMemset(b->d_ck_sync, 0, sizeof(int) * (size_t)((nb_streams + 15) / 16)) == hipSuccess;
  ok = ok && hipMalloc(&b->d_lpc_tab, sizeof(LpcTables)) == hipSuccess;
  /* d_chunk (the chunked path's frame outputs, LPC_CHUNK x 4.9 KB per
   * stream) is allocated by the first call that takes that path */
  if (ok) {
    LpcTables T;
    build_lpc_tables(T);
    ok = hipMemcpy(b->d_lpc_tab, &T, sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
  }
  if (ok && nb_streams <= OVERLAP_MAX_STREAMS) {
    ok = ok && hipStreamCreateWithFlags(&b->fstream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&b->ev_start, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 2 && ok; i++) {
      ok = ok && hipMalloc(&b->d_cond[i], sizeof(FrameCond) * (size_t)nb_streams) == hipSuccess;
      ok = ok && hipEventCreateWithFlags(&b->ev_frame[i], hipEventDisableTiming) == hipSuccess;
      ok = ok && hipEventCreateWithFlags(&b->ev_samp[i], hipEventDisableTiming) == hipSuccess;
    }
  }
  if (!ok) {
    set_err("device allocation failed");
    lpcnet_batch_destroy(b);
    return nullptr;
  }
  if (const char *km = getenv("LPCNET_KERNEL")) b->kernel_mode = atoi(km);
  lpcnet_batch_reset(b);
  return b;
}

LPCNET_EXPORT void lpcnet_batch_destroy(LPCNetBatch *b)
{
  if (!b) return;
  b->set_device();
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  if (b->fstream) (void)hipStreamSynchronize(b->fstream);
  conceal_free(b);
  free_model(b);
  plc_free(b);
  feat_free(b);
  (void)hipFree(b->d_state);
  (void)hipFree(b->d_ck_sync);
  (void)hipFree(b->d_feat);
  (void)hipFree(b->d_pcm);
  (void)hipFree(b->d_trace_logits);
  (void)hipFree(b->d_trace_exc);
  (void)hipFree(b->d_stamps);
  (void)hipFree(b->d_lpc);
  (void)hipFree(b->d_lpc_tab);
  (void)hipFree(b->d_chunk);
  if (b->io_feat_vram) (void)hipFree(b->h_io_feat);
  else (void)hipHostFree(b->h_io_feat);
  (void)hipHostFree(b->h_io_pcm);
  (void)hipHostFree(b->h_stg_feat);
  (void)hipHostFree(b->h_stg_pcm);
  if (b->ev_tick) (void)hipEventDestroy(b->ev_tick);
  (void)hipFree(b->d_packets);
  (void)hipFree(b->d_dfeat);
  (void)hipFree(b->d_dpcm);
  for (int i = 0; i < 2; i++) {
    (void)hipFree(b->d_cond[i]);
    if (b->ev_frame[i]) (void)hipEventDestroy(b->ev_frame[i]);
    if (b->ev_samp[i]) (void)hipEventDestroy(b->ev_samp[i]);
  }
  if (b->h_status) (void)hipHostFree(b->h_status);
  if (b->ev_start) (void)hipEventDestroy(b->ev_start);
  if (b->fstream) (void)hipStreamDestroy(b->fstream);
  for (hipEvent_t e : b->ev_taken) (void)hipEventDestroy(e);
  for (hipEvent_t e : b->ev_free) (void)hipEventDestroy(e);
  if (b->stream) (void)hipStreamDestroy(b->stream);
  delete b;
}

LPCNET_EXPORT int lpcnet_batch_load_model(LPCNetBatch *b, const unsigned char *data, int len)
{
  if (!b) return -1;
  if (b->set_device()) return -1;
  (void)hipStreamSynchronize(b->stream);
  conceal_free(b); /* its buffers are laid out for the model it was opened on */
  /* the batch's own copy of the blob, which its host model looks into */
  std::vector<unsigned char> blob;
  if (data && len > 0) blob.assign(data, data + len);
  auto host = std::make_unique<HostModel>();
  const int rc = load_model(b, blob.data(), len, *host);
  if (rc == 0) {
    b->blob.swap(blob);
    b->host = std::move(host);
    plc_load(b, b->host->records); /* optional records: a blob without them loads as ever */
  } else if (!b->have_model) {
    plc_free(b);
    b->plc_why = "no model loaded";
  }
  return rc;
}

/* after a change of the kernel mode or the rcpps table: re-plan the register
 * tables when the wide kernel's plan class no longer matches the choice
 * (speed only; the stream states, the model constants and the rcpps table
 * stay: load_model's replan form).  A re-plan that fails (a device
 * allocation or upload) has changed nothing in the batch: the previous,
 * correct tables and their plan class stay, and the setter succeeds. */
static int replan_if_needed(LPCNetBatch *b)
{
  if (!b->have_model || !b->caps.mf_ok || b->blob.empty() ||
      wide_now(b->B, b->kernel_mode, b->rcp_custom, b->plan.cus) == b->plan_wide)
    return 0;
  if (b->set_device()) return -1;
  (void)hipStreamSynchronize(b->stream);
  auto host = std::make_unique<HostModel>();
  if (load_model(b, b->blob.data(), (int)b->blob.size(), *host, true) == 0) b->host = std::move(host);
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_set_kernel(LPCNetBatch *b, int mode)
{
  if (!b || !(mode == 0 || mode == 1 || mode == 4 || mode == 5)) {
    set_err("kernel mode must be 0 (auto), 1 (lockstep), 4 (mf_kernel) or 5 (fp_kernel)");
    return -1;
  }
  b->kernel_mode = mode;
  if (b->have_model) plan_batch(b);
  return replan_if_needed(b);
}

LPCNET_EXPORT int lpcnet_batch_set_model_constants(LPCNetBatch *b, float lpc_gamma, int features_delay, int end2end)
{
  if (!b || !b->have_model) { set_err("no model loaded"); return -1; }
  const ModelConst mc{lpc_gamma, features_delay, end2end};
  if (check_constants(mc)) return -1;
  if (b->set_device()) return -1;
  (void)hipStreamSynchronize(b->stream); /* queued frames keep the constants they were enqueued with */
  b->mc = mc;
  b->info.lpc_gamma = mc.lpc_gamma;
  b->info.features_delay = mc.delay;
  b->info.end2end = mc.end2end;
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_set_rcp_table(LPCNetBatch *b, const uint32_t *tab)
{
  if (!b || !b->have_model) { set_err("no model loaded"); return -1; }
  const std::vector<uint32_t> dflt = default_rcp_dev();
  std::vector<uint32_t> dev = dflt;
  for (int i = 0; i < RCP_ENTRIES && tab; i++) dev[i] = tab[i] + kRcpBias;
  if (b->set_device()) return -1;
  HIPCHK(hipStreamSynchronize(b->stream));
  /* the LDS image's table section and the frame network's global copy */
  HIPCHK(hipMemcpy((unsigned char *)b->sa.image + IMG_RCP, dev.data(), RCP_ENTRIES * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy((void *)b->fa.rcp, dev.data(), RCP_ENTRIES * 4, hipMemcpyHostToDevice));
  b->rcp_dev = dev;
  b->rcp_custom = dev != dflt;
  plan_batch(b);
  return replan_if_needed(b);
}

LPCNET_EXPORT int lpcnet_batch_model_info(const LPCNetBatch *b, LPCNetModelInfo *info)
{
  if (!b || !b->have_model || !info) return -1;
  *info = b->info;
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_nb_streams(const LPCNetBatch *b) { return b ? b->B : 0; }

LPCNET_EXPORT int lpcnet_batch_reset_stream(LPCNetBatch *b, int stream)
{
  if (!b || stream < 0 || stream >= b->B) return -1;
  if (b->set_device()) return -1;
  StreamState s;
  host_reset_state(s);
  HIPCHK(hipMemcpyAsync(&b->d_state[stream], &s, sizeof(s), hipMemcpyHostToDevice, b->stream));
  /* lpcnet_plc_reset clears plc_net with the synthesis state, and the
   * analysis state (lpcnet_encoder_init inside lpcnet_plc_reset) */
  if (side_reset(b, stream, SIDE_PLC | SIDE_FEAT) || conceal_reset_streams(b, stream)) return -1;
  HIPCHK(hipStreamSynchronize(b->stream));
  b->min_fc = std::min(b->min_fc, s.frame_count);
  return 0;
}

LPCNET_EXPORT void lpcnet_batch_reset(LPCNetBatch *b)
{
  if (!b || b->set_device()) return;
  std::vector<StreamState> v(b->B);
  host_reset_state(v[0]);
  for (int i = 1; i < b->B; i++) v[i] = v[0];
  (void)hipMemcpyAsync(b->d_state, v.data(), sizeof(StreamState) * v.size(), hipMemcpyHostToDevice, b->stream);
  (void)side_reset(b, -1, SIDE_PLC | SIDE_FEAT);
  (void)conceal_reset_streams(b, -1);
  (void)hipStreamSynchronize(b->stream);
  b->min_fc = v[0].frame_count;
}

/* One frame of a large batch in the chunked form (a live server's tick:
 * lpcnet_batch_synthesize once per 10 ms): lpc_kernel, chunk_kernel with
 * stream-only columns (weights fetched once per 16-32 streams instead of the
 * per-frame frame_kernel's once per 4: at 1024 streams ~44 -> ~20 us, at
 * 28 K streams 28 rounds of workgroups -> 2-4), then the sample kernel
 * reading the frame's conditioning, LPC and frame_count from the stream
 * state (no per-frame output copy: half the chunk kernel's stores).  Same
 * arithmetic as every other frame
 * path (the chunk kernel is bit-identical to the frame kernel).  Taken where
 * single_frame_chunked (kernel_choice.cpp) says so. */
/* d_features: device memory, or the mapped host buffer (mapped = true: a
 * deferred LPC then reads the chunk kernel's copy in b->d_feat) */
static int launch_single_frame_chunked(LPCNetBatch *b, int nB, const float *d_features, short *d_pcm, int N,
                                       bool defer = false, bool mapped = false)
{
  if (!b->mc.end2end && !defer && launch_lpc(d_features, b->d_lpc, nB, b->d_lpc_tab, b->stream)) {
    set_err("lpc kernel launch failed");
    return -1;
  }
  FrameArgs fa = b->fa;
  fa.st = b->d_state;
  fa.mc = b->mc;
  fa.nstreams = nB;
  fa.features = d_features;
  fa.lpc_new = b->d_lpc;
  fa.nframes = 1;
  fa.cond = nullptr;
  fa.stamps = nullptr;
  fa.lpc_defer = defer ? 1 : 0;
  fa.lpc_feat = defer && mapped ? b->d_feat : nullptr;
  fa.ck_sync = b->d_ck_sync;
  fa.status = b->d_status;
  hipEvent_t e0, e1, e2;
  if (mark(b, b->timing >= 2, b->stream, e0)) return -1;
  if (launch_chunk(fa, b->stream)) {
    set_err("chunk kernel launch failed");
    return -1;
  }
  b->frames_done(1);
  SampleArgs sa = sample_args(b, nB, N);
  sa.cond = nullptr;
  sa.nframes = 1;
  sa.pcm = d_pcm;
  if (mark(b, b->timing >= 1, b->stream, e1)) return -1;
  if (launch_sample_kernel(b, sa)) return -1;
  if (mark(b, b->timing >= 1, b->stream, e2)) return -1;
  timed(b, 1, e0, e1, 1);
  timed(b, 0, e1, e2, 1);
  return 0;
}

/* the batch's pinned host I/O buffers ([B][NF] features, [B][FRAME] PCM,
 * mapped: the kernels read and store them over PCIe) and the pinned staging
 * of callers' own buffers (cached, DMA) */
static int ensure_host_io(LPCNetBatch *b)
{
  if (!b->h_io_feat) {
    /* features: host-visible device memory where the device has a large BAR
     * (the host's stores cross PCIe as posted writes, the chunk and LPC
     * kernels then read local HBM: 80 KB at 1024 streams, the chunk kernel's
     * input phase ~24 K -> ~12 K cycles against reads of mapped host memory),
     * else mapped pinned host memory.  LPCNET_FEAT_VRAM=0: always the latter. */
    int large_bar = 0;
    (void)hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, b->device);
    const char *ev = getenv("LPCNET_FEAT_VRAM");
    if (large_bar && !(ev && atoi(ev) == 0) &&
        hipExtMallocWithFlags((void **)&b->h_io_feat, sizeof(float) * NF * (size_t)b->B, hipDeviceMallocFinegrained) ==
            hipSuccess) {
      b->io_feat_vram = true;
      b->d_io_feat = b->h_io_feat;
    } else {
      b->h_io_feat = nullptr;
      HIPCHK(hipHostMalloc(&b->h_io_feat, sizeof(float) * NF * (size_t)b->B, hipHostMallocMapped));
      HIPCHK(hipHostGetDevicePointer((void **)&b->d_io_feat, b->h_io_feat, 0));
    }
  }
  if (!b->h_io_pcm) {
    HIPCHK(hipHostMalloc(&b->h_io_pcm, sizeof(short) * FRAME * (size_t)b->B, hipHostMallocMapped));
    HIPCHK(hipHostGetDevicePointer((void **)&b->d_io_pcm, b->h_io_pcm, 0));
  }
  if (!b->h_stg_feat) HIPCHK(hipHostMalloc(&b->h_stg_feat, sizeof(float) * NF * (size_t)b->B, hipHostMallocDefault));
  if (!b->h_stg_pcm) HIPCHK(hipHostMalloc(&b->h_stg_pcm, sizeof(short) * FRAME * (size_t)b->B, hipHostMallocDefault));
  return 0;
}

/* the end of a synchronous call.  poll: the calling thread polls the
 * call's event (no sleep / wake-up between the last kernel and the thread's
 * next step), handing over to a blocking wait after TICK_SPIN_MS -- the
 * drop-in pool's combiner (64 C threads: 19-20 -> 27.5 M samples/s, 256:
 * 58-60 -> 69-84 M); otherwise hipStreamSynchronize, 2-3 % faster for one
 * caller driving a batch (tools/sync_ab.sh, profiles/r05/sync_ab.log).
 * LPCNET_SYNC_BLOCK=1 / LPCNET_SYNC_POLL=1 force one form everywhere. */
static int tick_sync(LPCNetBatch *b, bool poll, const std::function<int()> &after = std::function<int()>())
{
  if (getenv("LPCNET_SYNC_POLL")) poll = true;
  const bool block = !poll || getenv("LPCNET_SYNC_BLOCK");
  if (block && !after) {
    HIPCHK(hipStreamSynchronize(b->stream));
    return 0;
  }
  if (!b->ev_tick) HIPCHK(hipEventCreateWithFlags(&b->ev_tick, hipEventDisableTiming));
  HIPCHK(hipEventRecord(b->ev_tick, b->stream));
  /* work queued behind the tick's end (the deferred LPC): not waited for */
  if (after && after()) return -1;
  if (block) {
    HIPCHK(hipEventSynchronize(b->ev_tick));
    return 0;
  }
  static const int pause = getenv("LPCNET_SYNC_PAUSE") ? atoi(getenv("LPCNET_SYNC_PAUSE")) : TICK_POLL_PAUSE;
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t q = hipEventQuery(b->ev_tick);
    if (q == hipSuccess) return 0;
    if (q != hipErrorNotReady) HIPCHK(q);
    if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(TICK_SPIN_MS)) break;
    for (int k = 0; k < pause; k++) __builtin_ia32_pause(); /* fewer runtime queries */
  }
  HIPCHK(hipEventSynchronize(b->ev_tick));
  return 0;
}

/* copy kind of a feature copy to the device: the batch's own feature buffer
 * is fine-grained VRAM on large-BAR devices (ensure_host_io), not host memory */
static hipMemcpyKind own_feat_kind(const LPCNetBatch *b, const float *features)
{
  return features == b->h_io_feat && b->io_feat_vram ? hipMemcpyDefault : hipMemcpyHostToDevice;
}

}  // extern "C"

/* one frame for the first nB streams of a batch, host I/O ([nB][NF] in,
 * [nB][N] out) */
int lpcnet_mi355x::synth_first(LPCNetBatch *b, int nB, const float *features, short *pcm, int N, int preload,
                               const PreSync &pre, bool staged)
{
  if (!b || !b->have_model) { set_err("no model loaded"); return -1; }
  if (N < 0 || N > FRAME || !features || (N > 0 && !pcm) || preload < 0) { set_err("bad arguments"); return -1; }
  if (b->set_device()) return -1;
  if (ensure_trace(b, N)) return -1;
  /* the caller's stores into the VRAM feature buffer are write-combined:
   * drained before any command of this call can read them */
  if (features == b->h_io_feat && b->io_feat_vram) __builtin_ia32_sfence();
  /* a drop-in pool's step (staged / pre) never takes the one-frame chunked
   * form: no look at the environment there */
  const bool own_call = !staged && !pre;
  const ChoiceEnv env = own_call ? choice_env_from_env() : ChoiceEnv();
  if (own_call &&
      single_frame_chunked(b->plan, b->chunking, nB, N, preload, b->sa.trace_logits != nullptr, b->d_stamps != nullptr, env)) {
    /* the caller's buffers through pinned staging: both copies truly
     * asynchronous, one synchronisation per frame.  Features already in the
     * batch's own pinned buffer (lpcnet_batch_host_features) skip the host
     * copy; PCM into the batch's own pinned buffer (lpcnet_batch_host_pcm)
     * is stored there by the sample kernel itself when its write-out is
     * coalesced (no device-to-host copy, no host copy) */
    if (ensure_host_io(b)) return -1;
    /* the batch's own buffers (mapped): up to ZC_FEAT_MAX streams the LPC
     * and chunk kernels read the features straight from host memory (80 B
     * per stream over PCIe, no copy command and its start latency), larger
     * batches take one DMA copy; the caller's buffers: host copy into the
     * cached pinned staging, one DMA copy each way */
    const bool own_feat = features == b->h_io_feat, own_pcm = pcm == b->h_io_pcm;
    const bool zc_feat = own_feat && (nB <= ZC_FEAT_MAX || b->io_feat_vram) && !getenv("LPCNET_FEAT_DMA");
    if (!own_feat) memcpy(b->h_stg_feat, features, sizeof(float) * NF * nB);
    if (!zc_feat)
      HIPCHK(hipMemcpyAsync(b->d_feat, own_feat ? b->h_io_feat : b->h_stg_feat, sizeof(float) * NF * nB,
                            own_feat_kind(b, features), b->stream));
    const bool direct = own_pcm && pcm_store_coalesced(launch_kernel(b, nB, false, false), env);
    const bool defer = lpc_deferred(b->mc.delay, b->mc.end2end, env);
    if (launch_single_frame_chunked(b, nB, zc_feat ? b->d_io_feat : b->d_feat, direct ? b->d_io_pcm : b->d_pcm, N,
                                    defer, zc_feat))
      return -1;
    if (!direct)
      HIPCHK(hipMemcpyAsync(own_pcm ? b->h_io_pcm : b->h_stg_pcm, b->d_pcm, sizeof(short) * N * nB,
                            hipMemcpyDeviceToHost, b->stream));
    auto lpc_after = [&]() -> int {
      /* LPCNET_CK_WARM=1 (A/B, measured: no gain at 1024 streams): it also
       * warms every XCD's L2 with the chunk kernel's weights for the next tick */
      const char *cw = getenv("LPCNET_CK_WARM");
      const bool warm = cw && atoi(cw) != 0 && b->ck_warm.m[0];
      if (launch_lpc(b->d_feat, nullptr, nB, b->d_lpc_tab, b->stream, b->d_state, b->mc.delay,
                     warm ? &b->ck_warm : nullptr)) {
        set_err("deferred lpc kernel launch failed");
        return -1;
      }
      return 0;
    };
    if (tick_sync(b, false, defer ? std::function<int()>(lpc_after) : std::function<int()>())) return -1;
    if (check_status(b)) return -1;
    if (!own_pcm) memcpy(pcm, b->h_stg_pcm, sizeof(short) * N * nB);
    return 0;
  }
  /* everything below is ordered after work already queued on b->stream
   * (staged: the caller has queued the features / preload copies already) */
  if (!staged) {
    /* the batch's own feature buffer may be device memory (host-visible VRAM) */
    HIPCHK(hipMemcpyAsync(b->d_feat, features, sizeof(float) * NF * nB, own_feat_kind(b, features), b->stream));
    if (preload > 0 && N > 0)
      HIPCHK(hipMemcpyAsync(b->d_pcm, pcm, sizeof(short) * N * nB, hipMemcpyHostToDevice, b->stream));
  }
  if (launch_frame_step(b, b->d_feat, b->d_lpc, true, b->d_pcm, N, preload, -1, nB)) return -1;
  if (pre && pre()) return -1;
  if (N > 0) HIPCHK(hipMemcpyAsync(pcm, b->d_pcm, sizeof(short) * N * nB, hipMemcpyDeviceToHost, b->stream));
  if (tick_sync(b, pre || staged)) return -1;
  return check_status(b);
}

extern "C" {

LPCNET_EXPORT int lpcnet_batch_synthesize_impl(LPCNetBatch *b, const float *features, short *pcm, int N, int preload)
{
  return synth_first(b, b ? b->B : 0, features, pcm, N, preload);
}

LPCNET_EXPORT int lpcnet_batch_synthesize(LPCNetBatch *b, const float *features, short *pcm, int N)
{
  return lpcnet_batch_synthesize_impl(b, features, pcm, N, 0);
}

LPCNET_EXPORT float *lpcnet_batch_host_features(LPCNetBatch *b)
{
  if (!b || b->set_device() || ensure_host_io(b)) return nullptr;
  return b->h_io_feat;
}

LPCNET_EXPORT short *lpcnet_batch_host_pcm(LPCNetBatch *b)
{
  if (!b || b->set_device() || ensure_host_io(b)) return nullptr;
  return b->h_io_pcm;
}

static int ensure_decode_bufs(LPCNetBatch *b, bool host_io)
{
  if (!b->d_packets) HIPCHK(hipMalloc(&b->d_packets, (size_t)DEC_MAX_PACKETS * b->B * 8));
  if (!b->d_dfeat) HIPCHK(hipMalloc(&b->d_dfeat, sizeof(float) * NF * 4 * DEC_MAX_PACKETS * (size_t)b->B));
  if (host_io && !b->d_dpcm) HIPCHK(hipMalloc(&b->d_dpcm, sizeof(short) * 4 * FRAME * (size_t)b->B));
  return 0;
}

static int decode_ready(LPCNetBatch *b)
{
  if (!b || !b->have_model) { set_err("no model loaded"); return -1; }
  if (!b->has_codebooks) {
    set_err("lpcnet_decode: the model blob carries no ceps_codebook1/2/3 / ceps_codebook_diff4 records "
            "(1024x17, 1024x17, 1024x17, 4096x18 floats)");
    return -1;
  }
  return b->set_device();
}

}  // extern "C"

/* lpcnet_decode (lpcnet.c:310-319) on the first nB streams, host I/O:
 * packets [nB][8] -> pcm [nB][4 * FRAME] */
int lpcnet_mi355x::decode_first(LPCNetBatch *b, int nB, const unsigned char *packets, short *pcm, const PreSync &pre)
{
  if (decode_ready(b)) return -1;
  if (!packets || !pcm) { set_err("bad arguments"); return -1; }
  if (ensure_trace(b, FRAME) || ensure_decode_bufs(b, true)) return -1;
  HIPCHK(hipMemcpyAsync(b->d_packets, packets, (size_t)nB * 8, hipMemcpyHostToDevice, b->stream));
  DecodeArgs da = b->da;
  da.packets = b->d_packets;
  da.npackets = 1;
  da.nstreams = nB;
  da.st = b->d_state;
  da.features = b->d_dfeat;
  if (launch_decode(da, b->stream)) { set_err("decode kernel launch failed"); return -1; }
  /* for (k=0;k<4;k++) lpcnet_synthesize(&st->lpcnet_state, features[k], &pcm[k*FRAME_SIZE], FRAME_SIZE) */
  for (int f = 0; f < 4; f++)
    if (launch_frame_step(b, b->d_dfeat + (size_t)f * nB * NF, b->d_lpc, true, b->d_dpcm + (size_t)f * nB * FRAME, FRAME, 0,
                          -1, nB))
      return -1;
  if (pre && pre()) return -1;
  std::vector<short> tmp((size_t)4 * nB * FRAME);
  HIPCHK(hipMemcpyAsync(tmp.data(), b->d_dpcm, sizeof(short) * tmp.size(), hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  if (check_status(b)) return -1;
  for (int k = 0; k < nB; k++)
    for (int f = 0; f < 4; f++)
      memcpy(pcm + ((size_t)k * 4 + f) * FRAME, &tmp[((size_t)f * nB + k) * FRAME], sizeof(short) * FRAME);
  return 0;
}

extern "C" {

LPCNET_EXPORT int lpcnet_batch_decode(LPCNetBatch *b, const unsigned char *packets, short *pcm)
{
  return decode_first(b, b ? b->B : 0, packets, pcm);
}

LPCNET_EXPORT int lpcnet_batch_decode_frames(LPCNetBatch *b, const unsigned char *d_packets, short *d_pcm, int npackets)
{
  if (decode_ready(b)) return -1;
  if (!d_packets || !d_pcm || npackets < 0) { set_err("bad arguments"); return -1; }
  if (ensure_decode_bufs(b, false)) return -1;
  for (int p0 = 0; p0 < npackets; p0 += DEC_MAX_PACKETS) {
    const int np = std::min(DEC_MAX_PACKETS, npackets - p0);
    DecodeArgs da = b->da;
    da.packets = d_packets + (size_t)p0 * b->B * 8;
    da.npackets = np;
    da.nstreams = b->B;
    da.st = b->d_state;
    da.features = b->d_dfeat;
    /* queued behind every kernel that still reads d_dfeat (the previous
     * group's frame kernels precede the sample kernels on b->stream) */
    if (launch_decode(da, b->stream)) { set_err("decode kernel launch failed"); return -1; }
    if (lpcnet_batch_synthesize_frames(b, nullptr, b->d_dfeat, d_pcm + (size_t)4 * p0 * b->B * FRAME, 4 * np, FRAME))
      return -1;
  }
  return 0;
}

}  // extern "C"

/* lpcnet_synthesize_tail_impl on the first nB streams: the sample network on
 * the conditioning and LPC already in the stream states, no frame network */
int lpcnet_mi355x::tail_first(LPCNetBatch *b, int nB, short *pcm, int N, int preload, const PreSync &pre)
{
  if (!b || !b->have_model) { set_err("no model loaded"); return -1; }
  if (N < 0 || N > FRAME || (N > 0 && !pcm) || preload < 0) { set_err("bad arguments"); return -1; }
  if (N == 0) return 0;
  if (b->set_device()) return -1;
  if (ensure_trace(b, N)) return -1;
  if (preload > 0) HIPCHK(hipMemcpyAsync(b->d_pcm, pcm, sizeof(short) * N * nB, hipMemcpyHostToDevice, b->stream));
  if (tail_first_device(b, nB, b->d_pcm, N, preload)) return -1;
  if (pre && pre()) return -1;
  HIPCHK(hipMemcpyAsync(pcm, b->d_pcm, sizeof(short) * N * nB, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return check_status(b);
}

/* run_frame_network on the first nB streams (features [nB][NF]); keep_cond:
 * into the caller's locals as run_frame_network_flush does (lpcnet.c:134-144),
 * otherwise into the state's conditioning (lpcnet.c:275) */
int lpcnet_mi355x::frame_first(LPCNetBatch *b, int nB, const float *features, bool keep_cond, const PreSync &pre)
{
  if (!b || !b->have_model) { set_err("no model loaded"); return -1; }
  if (!features) { set_err("bad arguments"); return -1; }
  if (b->set_device()) return -1;
  HIPCHK(hipMemcpyAsync(b->d_feat, features, sizeof(float) * NF * nB, hipMemcpyHostToDevice, b->stream));
  if (frame_first_device(b, nB, b->d_feat, keep_cond)) return -1;
  if (pre && pre()) return -1;
  HIPCHK(hipStreamSynchronize(b->stream));
  return check_status(b);
}

/* ---- device-I/O siblings of the three steps above (batch.h) ----------------
 * launch_frame_step on nB states with device buffers: queued on b->stream,
 * no copy, no synchronisation, no look at the environment. */
namespace {

/* the states the launches of a step run on: the batch's own, or for the
 * scope of this object the caller's work states.  The batch's frame_count
 * bound is about its own states: a step on work states leaves it alone. */
struct StepStates {
  LPCNetBatch *b;
  StreamState *own;
  int min_fc;
  bool work;
  StepStates(LPCNetBatch *b_, StreamState *st) : b(b_), own(b_->d_state), min_fc(b_->min_fc), work(st != nullptr)
  {
    if (work) {
      b->d_state = st;
      b->min_fc = 0;
    }
  }
  ~StepStates()
  {
    b->d_state = own;
    if (work) b->min_fc = min_fc;
  }
};

int step_ready(LPCNetBatch *b, int nB, int N, int preload, bool need_pcm, const void *d_pcm)
{
  if (!b || !b->have_model) { set_err("no model loaded"); return -1; }
  if (nB < 1 || nB > b->B || N < 0 || N > FRAME || preload < 0 || (need_pcm && N > 0 && !d_pcm)) { set_err("bad arguments"); return -1; }
  return b->set_device();
}

}  // namespace

int lpcnet_mi355x::synth_first_device(LPCNetBatch *b, int nB, const float *d_features, short *d_pcm, int N, int preload,
                                      StreamState *st)
{
  if (step_ready(b, nB, N, preload, true, d_pcm)) return -1;
  if (!d_features) { set_err("bad arguments"); return -1; }
  if (ensure_trace(b, N)) return -1;
  StepStates on(b, st);
  return launch_frame_step(b, d_features, b->d_lpc, true, d_pcm, N, preload, -1, nB);
}

int lpcnet_mi355x::tail_first_device(LPCNetBatch *b, int nB, short *d_pcm, int N, int preload, StreamState *st)
{
  if (step_ready(b, nB, N, preload, true, d_pcm)) return -1;
  if (N == 0) return 0;
  if (ensure_trace(b, N)) return -1;
  StepStates on(b, st);
  return launch_frame_step(b, nullptr, nullptr, false, d_pcm, N, preload, -1, nB, false, false);
}

int lpcnet_mi355x::frame_first_device(LPCNetBatch *b, int nB, const float *d_features, bool keep_cond, StreamState *st)
{
  if (step_ready(b, nB, 0, 0, false, nullptr)) return -1;
  if (!d_features) { set_err("bad arguments"); return -1; }
  StepStates on(b, st);
  return launch_frame_step(b, d_features, b->d_lpc, true, nullptr, 0, 0, -1, nB, true, keep_cond);
}

extern "C" {

LPCNET_EXPORT int lpcnet_batch_synthesize_tail_impl(LPCNetBatch *b, short *pcm, int N, int preload)
{
  return tail_first(b, b ? b->B : 0, pcm, N, preload);
}

LPCNET_EXPORT int lpcnet_batch_run_frame_network(LPCNetBatch *b, const float *features, int update_conditions)
{
  return frame_first(b, b ? b->B : 0, features, update_conditions == 0);
}

LPCNET_EXPORT int lpcnet_batch_reset_signal(LPCNetBatch *b, int stream)
{
  if (!b || stream < 0 || stream >= b->B) { set_err("bad arguments"); return -1; }
  if (b->set_device()) return -1;
  StreamState s;
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipMemcpy(&s, &b->d_state[stream], sizeof(s), hipMemcpyDeviceToHost));
  reset_signal(s);
  HIPCHK(hipMemcpy(&b->d_state[stream], &s, sizeof(s), hipMemcpyHostToDevice));
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_state_size(void) { return (int)sizeof(StreamState); }

LPCNET_EXPORT int lpcnet_batch_save_state(LPCNetBatch *b, int stream, void *buf)
{
  if (!b || stream < 0 || stream >= b->B || !buf || b->set_device()) return -1;
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipMemcpy(buf, &b->d_state[stream], sizeof(StreamState), hipMemcpyDeviceToHost));
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_restore_state(LPCNetBatch *b, int stream, const void *buf)
{
  if (!b || stream < 0 || stream >= b->B || !buf || b->set_device()) return -1;
  if (!snapshot_ok(buf)) return -1;
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipMemcpy(&b->d_state[stream], buf, sizeof(StreamState), hipMemcpyHostToDevice));
  int fc;
  memcpy(&fc, (const unsigned char *)buf + offsetof(StreamState, frame_count), sizeof(fc));
  b->min_fc = std::min(b->min_fc, fc);
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_synthesize_frames(LPCNetBatch *b, const float *h_features, const float *d_features,
                                                 short *d_pcm, int nframes, int N)
{
  (void)h_features; /* kept for ABI compatibility: lpc_from_cepstrum now runs on the device */
  if (!b || !b->have_model) { set_err("no model loaded"); return -1; }
  if (N < 0 || N > FRAME || nframes < 0 || !d_features || !d_pcm) { set_err("bad arguments"); return -1; }
  if (b->set_device()) return -1;
  if (ensure_trace(b, N)) return -1;
  const size_t fstride = (size_t)b->B * NF;
  if (nframes == 0) return 0;
  const FramePath path = frame_path(b->plan, b->B, b->fstream != nullptr, b->chunking, b->sa.trace_logits != nullptr,
                                    b->d_stamps != nullptr, nframes, N, choice_env_from_env());
  const bool mfm = path.multi_frame, ovl = path.overlapped, chunked = path.chunked;
  if (ovl) {
    /* the first frame kernel follows everything already on stream */
    HIPCHK(hipEventRecord(b->ev_start, b->stream));
    HIPCHK(hipStreamWaitEvent(b->fstream, b->ev_start, 0));
  }
  if (chunked && !b->d_chunk) {
    /* frame-network outputs of a chunk of frames (chunk_kernel -> sample
     * launches): sizeof(FrameCond) = 4.9 KB x LPC_CHUNK per stream (160 MB
     * at 1024 streams), only for batches that take this path */
    if (hipMalloc(&b->d_chunk, sizeof(FrameCond) * (size_t)LPC_CHUNK * b->B) != hipSuccess) {
      b->d_chunk = nullptr;
      set_err("device allocation of the chunked frame-network buffer failed");
      return -1;
    }
  }
  hipStream_t fs = ovl ? b->fstream : b->stream;
  for (int c0 = 0; c0 < nframes; c0 += LPC_CHUNK) {
    /* lpc_from_cepstrum depends only on the features: one launch for up to
     * LPC_CHUNK frames x B streams fills the GPU (a per-frame launch of B
     * one-wave streams is latency-bound); queued on the frame kernels' queue,
     * after the frame kernels of the previous chunk that read d_lpc */
    const int n = std::min(LPC_CHUNK, nframes - c0);
    if (!b->mc.end2end && launch_lpc(d_features + c0 * fstride, b->d_lpc, n * b->B, b->d_lpc_tab, fs)) {
      set_err("lpc kernel launch failed");
      return -1;
    }
    if (chunked && n >= CHUNK_MIN_FRAMES) {
      const int fc0 = b->min_fc;
      if (launch_chunk_frames(b, d_features + c0 * fstride, n)) return -1;
      /* frames in which a stream may still turn active: one launch each */
      const int k = mfm ? std::min(n, std::max(0, b->mc.delay - fc0)) : n;
      for (int f = c0; f < c0 + k; f++)
        if (launch_chunk_samples(b, f - c0, d_pcm + (size_t)f * b->B * N, N)) return -1;
      if (k < n && launch_chunk_samples(b, k, d_pcm + (size_t)(c0 + k) * b->B * N, N, n - k)) return -1;
      continue;
    }
    for (int f = c0; f < c0 + n; f++)
      if (launch_frame_step(b, d_features + f * fstride, b->d_lpc + (size_t)(f - c0) * b->B * NLPC, false,
                            d_pcm + (size_t)f * b->B * N, N, 0, ovl ? f : -1))
        return -1;
  }
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_sync(LPCNetBatch *b)
{
  if (!b || b->set_device()) return -1;
  HIPCHK(hipStreamSynchronize(b->stream));
  return check_status(b);
}

LPCNET_EXPORT int lpcnet_batch_set_frame_chunking(LPCNetBatch *b, int enable)
{
  if (!b) return -1;
  b->chunking = enable != 0;
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_set_spin_limit(LPCNetBatch *b, int polls)
{
  if (!b || polls < 0) return -1;
  /* clamped: the kernels' poll counter must be able to exceed the limit */
  b->spin_limit = polls == 0 ? FLAG_SPIN_LIMIT_DEFAULT : std::min(polls, FLAG_SPIN_LIMIT_MAX);
  return 0;
}

LPCNET_EXPORT void *lpcnet_batch_device_alloc(LPCNetBatch *b, size_t bytes)
{
  if (!b || b->set_device()) return nullptr;
  void *p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) { set_err("hipMalloc failed"); return nullptr; }
  return p;
}

LPCNET_EXPORT int lpcnet_batch_device_free(LPCNetBatch *b, void *p)
{
  if (!b || b->set_device()) return -1;
  HIPCHK(hipFree(p));
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_memcpy_h2d(LPCNetBatch *b, void *dst, const void *src, size_t bytes)
{
  if (!b || b->set_device()) return -1;
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_memcpy_d2h(LPCNetBatch *b, void *dst, const void *src, size_t bytes)
{
  if (!b || b->set_device()) return -1;
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

LPCNET_EXPORT void lpcnet_batch_reset_timers(LPCNetBatch *b, int enable)
{
  if (!b) return;
  b->set_device();
  (void)hipStreamSynchronize(b->stream);
  for (int k = 0; k < TIMED_REGIONS; k++) {
    b->ev_pairs[k].clear();
    b->ev_frames[k].clear();
  }
  /* stream is idle (and fstream with it): no slot reuse needs a wait */
  b->ev_samp_used[0] = b->ev_samp_used[1] = false;
  for (hipEvent_t e : b->ev_taken) b->ev_free.push_back(e);
  b->ev_taken.clear();
  b->timing = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
}

LPCNET_EXPORT double lpcnet_batch_kernel_ms(LPCNetBatch *b, int which, int *launches)
{
  if (!b || which < 0 || which >= TIMED_REGIONS) return -1;
  b->set_device();
  (void)hipStreamSynchronize(b->stream);
  double tot = 0;
  const std::vector<hipEvent_t> &v = b->ev_pairs[which];
  for (size_t i = 0; i + 1 < v.size(); i += 2) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, v[i], v[i + 1]) == hipSuccess) tot += ms;
  }
  if (launches) *launches = (int)(v.size() / 2);
  return tot;
}

LPCNET_EXPORT int lpcnet_batch_kernel_frames(LPCNetBatch *b, int which)
{
  if (!b || which < 0 || which >= TIMED_REGIONS) return -1;
  int n = 0;
  for (int k : b->ev_frames[which]) n += k;
  return n;
}

static int stamp_groups(const LPCNetBatch *b)
{
  const int spw = std::max(1, b->info.streams_per_workgroup);
  return (b->B + spw - 1) / spw;
}

LPCNET_EXPORT int lpcnet_batch_set_stamps(LPCNetBatch *b, int enable)
{
  if (!b || b->set_device()) return -1;
  (void)hipStreamSynchronize(b->stream);
  if (b->d_stamps) (void)hipFree(b->d_stamps);
  b->d_stamps = nullptr;
  if (enable) {
    /* sample kernel [groups][STAMP_WAVES][16] (enough for any S), then the
     * frame kernel [B / FRAME_STREAMS][16] */
    size_t n = (size_t)b->B * STAMP_WAVES * 16 + (size_t)(frame_groups(b->B) + 1) * 16;
    HIPCHK(hipMalloc(&b->d_stamps, n * 8));
    HIPCHK(hipMemset(b->d_stamps, 0, n * 8));
  }
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_get_stamps(LPCNetBatch *b, unsigned long long *out)
{
  if (!b || !b->d_stamps || !b->have_model || b->set_device()) return -1;
  HIPCHK(hipStreamSynchronize(b->stream));
  int g = stamp_groups(b);
  HIPCHK(hipMemcpy(out, b->d_stamps, (size_t)g * STAMP_WAVES * 16 * 8, hipMemcpyDeviceToHost));
  return g;
}

LPCNET_EXPORT int lpcnet_batch_get_frame_stamps(LPCNetBatch *b, unsigned long long *out)
{
  if (!b || !b->d_stamps || !b->have_model || b->set_device()) return -1;
  HIPCHK(hipStreamSynchronize(b->stream));
  const int g = frame_groups(b->B);
  HIPCHK(hipMemcpy(out, b->d_stamps + (size_t)b->B * STAMP_WAVES * 16, (size_t)g * 16 * 8, hipMemcpyDeviceToHost));
  return g;
}

LPCNET_EXPORT int lpcnet_batch_set_trace(LPCNetBatch *b, int enable)
{
  if (!b) return -1;
  b->trace = enable != 0;
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_get_trace(LPCNetBatch *b, float *logits, int *exc)
{
  if (!b || !b->trace || !b->d_trace_logits || b->set_device()) return -1;
  HIPCHK(hipStreamSynchronize(b->stream));
  int N = b->trace_N;
  if (logits) HIPCHK(hipMemcpy(logits, b->d_trace_logits, sizeof(float) * 8 * N * b->B, hipMemcpyDeviceToHost));
  if (exc) HIPCHK(hipMemcpy(exc, b->d_trace_exc, sizeof(int) * N * b->B, hipMemcpyDeviceToHost));
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_get_state(LPCNetBatch *b, int stream, float *gru_a_cond, float *gru_b_cond, float *lpc,
                                         float *gru_a_state, float *gru_b_state, int *frame_count)
{
  if (!b || stream < 0 || stream >= b->B || b->set_device()) return -1;
  StreamState s;
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipMemcpy(&s, &b->d_state[stream], sizeof(s), hipMemcpyDeviceToHost));
  if (gru_a_cond) memcpy(gru_a_cond, s.gru_a_cond, sizeof(s.gru_a_cond));
  if (gru_b_cond) memcpy(gru_b_cond, s.gru_b_cond, sizeof(s.gru_b_cond));
  if (lpc) memcpy(lpc, s.lpc, sizeof(s.lpc));
  if (gru_a_state) memcpy(gru_a_state, s.gru_a_state, sizeof(s.gru_a_state));
  if (gru_b_state) memcpy(gru_b_state, s.gru_b_state, sizeof(s.gru_b_state));
  if (frame_count) *frame_count = s.frame_count;
  return 0;
}

/* Host-only check of a weight blob against every rule lpcnet_load_model
 * applies (no device needed). */
LPCNET_EXPORT int lpcnet_mi355x_validate_model(const unsigned char *data, int len)
{
  /* diagnostics: the batch size whose kernel plan to build (LPCNET_VERBOSE prints it) */
  const char *v = getenv("LPCNET_VALIDATE_STREAMS");
  const int B = v ? std::max(1, atoi(v)) : 1;
  HostModel host;
  return build_host_model(data, len, build_opts(B, wide_now(B, 0, false, current_device_cus())), host);
}

/* fixed order: the SampleArgs block, the MODEL_TABLES upload entries (0: not
 * part of this model), ck_rep, the kernel-choice scalars, the work numbers */
LPCNET_EXPORT int lpcnet_mi355x_model_digest(const unsigned char *data, int len, int streams, int cus, int wide, uint64_t *out,
                                             int cap)
{
  if (!out || cap < MODEL_TABLES + 4 || streams < 1) { set_err("bad arguments"); return -1; }
  HostModel h;
  if (build_host_model(data, len, build_opts(streams, wide < 0 ? wide_now(streams, 0, false, cus) : wide != 0), h)) return -1;
  ModelArgs args;
  int n = 0;
  out[n++] = fnv1a64(&h.sa, sizeof(h.sa));
  for (const ModelUpload &u : model_uploads(h, args)) out[n++] = u.present ? fnv1a64(u.src, u.bytes) : 0;
  out[n++] = fnv1a64(h.ck_rep, sizeof(h.ck_rep));
  const int sc[] = {h.variant, h.sat, h.reg, h.mf_ok, h.fp_ok, h.cb_ok, h.plan_wide, h.rcp_custom, h.S, h.lds, h.nba, h.nbb};
  out[n++] = fnv1a64(sc, sizeof(sc));
  const double wk[] = {h.info.bytes_shared_per_frame, h.info.bytes_shared_per_sample, h.info.bytes_per_stream_sample,
                       h.info.ops_per_sample, h.mf_ga_ops, h.mf_gb_ops};
  out[n++] = fnv1a64(wk, sizeof(wk));
  return n;
}

/* the choice of a batch of `streams` streams on a device of `cus` compute
 * units (0: the current device's, the one case that asks a device) under the
 * current environment: the host model as a load builds it, its plan, and
 * kernel_choice.cpp's answer per launch row and per call row
 * (include/lpcnet_mi355x.h gives the layouts) */
LPCNET_EXPORT int lpcnet_mi355x_kernel_choice(const unsigned char *data, int len, int streams, int cus, int kernel_mode,
                                              int rcp_custom, int *plan, const int *launches, int nlaunches, int *launch_out,
                                              const int *calls, int ncalls, int *call_out)
{
  if (!plan || streams < 1 || cus < 0 || nlaunches < 0 || ncalls < 0 || (nlaunches && (!launches || !launch_out)) ||
      (ncalls && (!calls || !call_out))) {
    set_err("bad arguments");
    return -1;
  }
  if (cus == 0) cus = current_device_cus();
  const ChoiceEnv env = choice_env_from_env();
  const bool wide = plans_wide(streams, kernel_mode, rcp_custom != 0, cus, env);
  HostModel h;
  if (build_host_model(data, len, build_opts(streams, wide), h)) return -1;
  const ModelCaps caps = model_caps(h);
  const SamplePlan p = plan_sample_kernels(caps, lds_sizes(caps), streams, cus, kernel_mode, rcp_custom != 0, env);
  const int pl[LPCNET_CHOICE_PLAN] = {(int)p.base, p.mf2, p.mfw, p.mfw_g, p.mfw_forced, h.plan_wide, p.rcp_hw, p.quad_path,
                                      p.streams_per_workgroup, p.lds_bytes, (int)p.mfma_ops_per_group_sample, wide, caps.mf_ok};
  memcpy(plan, pl, sizeof(pl));
  for (int i = 0; i < nlaunches; i++) {
    const int *r = launches + 4 * i;
    const SampleKernel k = kernel_for_launch(p, r[0], r[1] != 0, r[2] != 0, r[3] != 0);
    launch_out[2 * i] = (int)k;
    launch_out[2 * i + 1] = pcm_store_coalesced(k, env);
  }
  for (int i = 0; i < ncalls; i++) {
    const int *r = calls + 10 * i;
    const FramePath f = frame_path(p, streams, r[5] != 0, r[4] != 0, r[6] != 0, r[7] != 0, r[0], r[1], env);
    int *o = call_out + 5 * i;
    o[0] = f.multi_frame;
    o[1] = f.overlapped;
    o[2] = f.chunked;
    o[3] = single_frame_chunked(p, r[4] != 0, r[2], r[1], r[3], r[6] != 0, r[7] != 0, env);
    o[4] = lpc_deferred(r[8], r[9], env);
  }
  return cus;
}

}  // extern "C"
