/*
 * synth_steps.cpp -- the step layer of a batch: the launches of one frame
 * step (lpc_kernel, frame_kernel or chunk_kernel, the sample kernel the plan
 * names) on the batch's HIP stream -- the first two on a second stream, one
 * frame ahead, for small batches -- and every synthesis and decode call built
 * on them: the batch entry points lpcnet_batch_synthesize*, _decode*,
 * _run_frame_network and _host_* of include/lpcnet_mi355x.h, and the
 * partial-batch steps of batch.h that dropin.cpp runs on a pool's work batch
 * and conceal_calls.cpp on its work states.  Which sample kernel and which
 * frame path a call takes is decided in kernel_choice.cpp (host-only): this
 * file fills its arguments and acts on the answer.  The batch itself -- its
 * lifecycle, model, setters, state and diagnostics -- is engine.cpp.
 * Compile with -ffp-contract=off, as every translation unit.
 */
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <string>
#include <vector>

#include "batch.h"

namespace {

/* ---- the sample kernel of a launch ---------------------------------------- */
/* What every sample launch takes from the batch: N samples for the nB states
 * at st.  Callers set cond, nframes, pcm, preload and stamps. */
SampleLaunch sample_args(const LPCNetBatch *b, StreamState *st, int nB, int N)
{
  SampleLaunch sa{};
  sa.st = st;
  sa.delay = b->mc.delay;
  sa.nstreams = nB;
  sa.N = N;
  sa.preload = 0;
  sa.stamps = nullptr;
  sa.trace_logits = b->trace_logits;
  sa.trace_exc = b->trace_exc;
  sa.status = b->d_status;
  sa.spin_limit = b->spin_limit;
  return sa;
}

/* What every frame or chunk launch takes from the batch: the frame network of
 * the nB states at st on d_features, its LPC in d_lpc.  Callers set nframes,
 * cond, stamps, keep_cond and the one-frame chunked form's fields. */
FrameArgs frame_args(const LPCNetBatch *b, StreamState *st, int nB, const float *d_features, float *d_lpc)
{
  FrameArgs fa = b->fa;
  fa.st = st;
  fa.mc = b->mc;
  fa.nstreams = nB;
  fa.features = d_features;
  fa.lpc_new = d_lpc;
  return fa;
}

/* the kernel a launch of the batch's first nB streams runs (the trace is the
 * batch's: ensure_trace) */
SampleKernel launch_kernel(const LPCNetBatch *b, int nB, bool preload, bool stamps)
{
  return kernel_for_launch(b->plan, nB, preload, b->trace_logits != nullptr, stamps);
}

int launch_sample_kernel(LPCNetBatch *b, const SampleLaunch &sa)
{
  if (sa.N <= 0) return 0;
  const SampleTables &t = b->sample; /* each kernel: the launch, the model part, its family's tables */
  int rc = -1;
  switch (launch_kernel(b, sa.nstreams, sa.preload != 0, sa.stamps != nullptr)) {
  case SampleKernel::FP: rc = launch_fp(FpArgs{sa, t.model, t.fp}, t.form, b->stream); break;
  case SampleKernel::MFW: rc = launch_mfw(MfwArgs{sa, t.model, t.mf, t.mfw}, t.form, b->plan.mfw_g, b->stream); break;
  case SampleKernel::MF2: rc = launch_mf2(MfArgs{sa, t.model, t.mf}, t.form, b->stream); break;
  case SampleKernel::MF:
    rc = launch_mf(MfArgs{sa, t.model, t.mf}, t.form, b->caps.S, mf_lds_bytes(b->caps.S, t.form.mf_split), b->stream);
    break;
  case SampleKernel::LOCKSTEP:
    rc = launch_sample(LockstepArgs{t.model, t.lockstep, sa}, b->caps.S, b->variant, b->sat ? 1 : 0, b->caps.reg ? 1 : 0,
                       b->caps.lds_bytes, b->stream);
    break;
  }
  if (rc) {
    set_err(std::string("sample kernel launch failed: ") + hipGetErrorString(hipGetLastError()));
    return -1;
  }
  return 0;
}

/* One frame step: the frame network of a frame, then N samples of it. */
struct FrameStep {
  /* the states the step runs on (null: the batch's own) and how many of them
   * (< 0: all B; fewer: the drop-in pool's work batch, the concealment
   * machine's work states) */
  StreamState *st = nullptr;
  int nB = -1;
  const float *d_features = nullptr;
  /* this frame's lpc_from_cepstrum output ([B][NLPC]); with run_lpc the LPC
   * kernel computing it is launched first, otherwise it was computed earlier
   * on the same queue (lpcnet_batch_synthesize_frames batches it over many
   * frames) */
  float *d_lpc_frame = nullptr;
  bool run_lpc = false;
  short *d_pcm = nullptr;
  int N = 0;
  int preload = 0;
  /* ovl >= 0: overlapped form, frame f = ovl, on the batch's own states, all
   * B of them.  The frame kernel runs on fstream, followed by a copy of its
   * outputs into d_cond[f & 1] (which sample kernel f-2 read: ev_samp); the
   * sample kernel on stream waits only for that copy (ev_frame) and reads the
   * frame's outputs there, so frame kernel f+1 runs beside sample kernel f.
   * The sample kernels read nothing else the frame kernel writes.  Every
   * fstream launch precedes a stream launch that waits for it, so a sync of
   * stream covers both. */
  int ovl = -1;
  /* run_frame false: the sample network only, on the conditioning already in
   * the stream states (lpcnet_synthesize_tail_impl, lpcnet.c:235-271);
   * keep_cond: the frame network of run_frame_network_flush (lpcnet.c:134-144) */
  bool run_frame = true;
  bool keep_cond = false;
};

/* The batch's frame_count bound (min_fc) is about its own states: a step on
 * other states leaves it alone. */
int launch_frame_step(LPCNetBatch *b, const FrameStep &s)
{
  const bool own = !s.st || s.st == b->d_state;
  const int ovl = s.ovl, N = s.N;
  if (ovl >= 0 && !own) { set_err("an overlapped frame step runs on the batch's own states only"); return -1; }
  StreamState *st = own ? b->d_state : s.st;
  const int nB = s.nB < 0 || ovl >= 0 ? b->B : s.nB;
  const bool run_frame = s.run_frame;
  const int c = ovl & 1;
  hipStream_t fs = ovl >= 0 ? b->fstream : b->stream;
  FrameArgs fa = frame_args(b, st, nB, s.d_features, s.d_lpc_frame);
  fa.keep_cond = s.keep_cond ? 1 : 0;
  SampleLaunch sa = sample_args(b, st, nB, N);
  sa.pcm = s.d_pcm;
  sa.preload = std::max(0, std::min(s.preload, N));
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
  if (run_frame && s.run_lpc && !b->mc.end2end && launch_lpc(s.d_features, s.d_lpc_frame, nB, b->d_lpc_tab, fs)) {
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
  timed(b, TIMED_FRAME, e0, ef ? ef : e1, 1);
  timed(b, TIMED_SAMPLE, e1, e2, 1);
  if (run_frame && own) b->frames_done(1);
  return 0;
}

/* Chunked form: the frame network of frames [0, n) of d_features has run
 * (chunk_kernel, outputs in d_chunk[f]); launch the sample kernel of frames
 * f .. f + nfr - 1 on b->stream, reading their conditioning from d_chunk[f..]
 * and writing d_pcm [nfr][B][N].  nfr > 1: matrix-core kernel only, every
 * stream past its first `delay` frames (SampleLaunch::nframes). */
int launch_chunk_samples(LPCNetBatch *b, int f, short *d_pcm, int N, int nfr = 1)
{
  SampleLaunch sa = sample_args(b, b->d_state, b->B, N);
  sa.cond = b->d_chunk + (size_t)f * b->B;
  sa.nframes = nfr;
  sa.pcm = d_pcm;
  sa.stamps = b->d_stamps;
  return timed_launch(b, TIMED_SAMPLE, b->timing >= 1, nfr, nullptr, [&] { return launch_sample_kernel(b, sa); });
}

/* Chunked form: the frame network of n frames (features [n][B][NF], their
 * LPC already in d_lpc) in one launch on b->stream. */
int launch_chunk_frames(LPCNetBatch *b, const float *d_features, int n)
{
  FrameArgs fa = frame_args(b, b->d_state, b->B, d_features, b->d_lpc);
  fa.nframes = n;
  fa.cond = b->d_chunk;
  fa.stamps = nullptr;
  if (timed_launch(b, TIMED_FRAME, b->timing >= 2, n, "chunk kernel launch failed", [&] { return launch_chunk(fa, b->stream); })) return -1;
  b->frames_done(n);
  return 0;
}

/* what a one-frame step checks before anything is queued, host or device
 * I/O: a model, nB of the batch's streams, N samples of a frame, and PCM to
 * take them where the step has any; makes the batch's device current */
int step_ready(LPCNetBatch *b, int nB, int N, int preload, bool need_pcm, const void *pcm)
{
  if (!b || !b->have_model) { set_err("no model loaded"); return -1; }
  if (nB < 1 || nB > b->B || N < 0 || N > FRAME || preload < 0 || (need_pcm && N > 0 && !pcm)) { set_err("bad arguments"); return -1; }
  return b->set_device();
}

}  // namespace

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
  FrameArgs fa = frame_args(b, b->d_state, nB, d_features, b->d_lpc);
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
  SampleLaunch sa = sample_args(b, b->d_state, nB, N);
  sa.cond = nullptr;
  sa.nframes = 1;
  sa.pcm = d_pcm;
  if (mark(b, b->timing >= 1, b->stream, e1)) return -1;
  if (launch_sample_kernel(b, sa)) return -1;
  if (mark(b, b->timing >= 1, b->stream, e2)) return -1;
  timed(b, TIMED_FRAME, e0, e1, 1);
  timed(b, TIMED_SAMPLE, e1, e2, 1);
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
    if (large_bar && !(ev && atoi(ev) == 0) && b->io_feat_dev.alloc_finegrained(NF * (size_t)b->B) == 0) {
      b->io_feat_vram = true;
      b->h_io_feat = b->d_io_feat = b->io_feat_dev;
    } else {
      if (b->io_feat_host.alloc(NF * (size_t)b->B, true)) return -1;
      HIPCHK(hipHostGetDevicePointer((void **)&b->d_io_feat, b->io_feat_host, 0));
      b->h_io_feat = b->io_feat_host;
    }
  }
  if (!b->h_io_pcm) {
    if (b->h_io_pcm.alloc(FRAME * (size_t)b->B, true)) return -1;
    HIPCHK(hipHostGetDevicePointer((void **)&b->d_io_pcm, b->h_io_pcm, 0));
  }
  if (!b->h_stg_feat && b->h_stg_feat.alloc(NF * (size_t)b->B, false)) return -1;
  if (!b->h_stg_pcm && b->h_stg_pcm.alloc(FRAME * (size_t)b->B, false)) return -1;
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
  if (!b->ev_tick && b->ev_tick.create(false)) return -1;
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

/* one frame for the first nB streams of a batch, host I/O ([nB][NF] in,
 * [nB][N] out) */
int lpcnet_mi355x::synth_first(LPCNetBatch *b, int nB, const float *features, short *pcm, int N, int preload,
                               const PreSync &pre, bool staged)
{
  if (step_ready(b, nB, N, preload, true, pcm)) return -1;
  if (!features) { set_err("bad arguments"); return -1; }
  if (ensure_trace(b, N)) return -1; /* the choice below asks about the trace */
  /* the caller's stores into the VRAM feature buffer are write-combined:
   * drained before any command of this call can read them */
  if (features == b->h_io_feat && b->io_feat_vram) __builtin_ia32_sfence();
  /* a drop-in pool's step (staged / pre) never takes the one-frame chunked
   * form: no look at the environment there */
  const bool own_call = !staged && !pre;
  const ChoiceEnv env = own_call ? choice_env_from_env() : ChoiceEnv();
  if (own_call &&
      single_frame_chunked(b->plan, b->chunking, nB, N, preload, b->trace_logits != nullptr, b->d_stamps != nullptr, env)) {
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
  if (synth_first_device(b, nB, b->d_feat, b->d_pcm, N, preload)) return -1;
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
  if (!b->d_packets && b->d_packets.alloc((size_t)DEC_MAX_PACKETS * b->B * 8)) return -1;
  if (!b->d_dfeat && b->d_dfeat.alloc((size_t)NF * 4 * DEC_MAX_PACKETS * b->B)) return -1;
  if (host_io && !b->d_dpcm && b->d_dpcm.alloc((size_t)4 * FRAME * b->B)) return -1;
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
  if (ensure_decode_bufs(b, true)) return -1;
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
    if (synth_first_device(b, nB, b->d_dfeat + (size_t)f * nB * NF, b->d_dpcm + (size_t)f * nB * FRAME, FRAME, 0)) return -1;
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
  if (step_ready(b, nB, N, preload, true, pcm)) return -1;
  if (N == 0) return 0;
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
  if (step_ready(b, nB, 0, 0, false, nullptr)) return -1;
  if (!features) { set_err("bad arguments"); return -1; }
  HIPCHK(hipMemcpyAsync(b->d_feat, features, sizeof(float) * NF * nB, hipMemcpyHostToDevice, b->stream));
  if (frame_first_device(b, nB, b->d_feat, keep_cond)) return -1;
  if (pre && pre()) return -1;
  HIPCHK(hipStreamSynchronize(b->stream));
  return check_status(b);
}

/* ---- device-I/O siblings of the three steps above (batch.h) ----------------
 * launch_frame_step on nB states with device buffers: queued on b->stream,
 * no copy, no synchronisation, no look at the environment. */
int lpcnet_mi355x::synth_first_device(LPCNetBatch *b, int nB, const float *d_features, short *d_pcm, int N, int preload,
                                      StreamState *st)
{
  if (step_ready(b, nB, N, preload, true, d_pcm)) return -1;
  if (!d_features) { set_err("bad arguments"); return -1; }
  if (ensure_trace(b, N)) return -1;
  FrameStep s;
  s.st = st;
  s.nB = nB;
  s.d_features = d_features;
  s.d_lpc_frame = b->d_lpc;
  s.run_lpc = true;
  s.d_pcm = d_pcm;
  s.N = N;
  s.preload = preload;
  return launch_frame_step(b, s);
}

int lpcnet_mi355x::tail_first_device(LPCNetBatch *b, int nB, short *d_pcm, int N, int preload, StreamState *st)
{
  if (step_ready(b, nB, N, preload, true, d_pcm)) return -1;
  if (N == 0) return 0;
  if (ensure_trace(b, N)) return -1;
  FrameStep s;
  s.st = st;
  s.nB = nB;
  s.d_pcm = d_pcm;
  s.N = N;
  s.preload = preload;
  s.run_frame = false;
  return launch_frame_step(b, s);
}

int lpcnet_mi355x::frame_first_device(LPCNetBatch *b, int nB, const float *d_features, bool keep_cond, StreamState *st)
{
  if (step_ready(b, nB, 0, 0, false, nullptr)) return -1;
  if (!d_features) { set_err("bad arguments"); return -1; }
  FrameStep s;
  s.st = st;
  s.nB = nB;
  s.d_features = d_features;
  s.d_lpc_frame = b->d_lpc;
  s.run_lpc = true;
  s.keep_cond = keep_cond;
  return launch_frame_step(b, s);
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
  const FramePath path = frame_path(b->plan, b->B, b->fstream != nullptr, b->chunking, b->trace_logits != nullptr,
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
    if (b->d_chunk.alloc((size_t)LPC_CHUNK * b->B)) {
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
    for (int f = c0; f < c0 + n; f++) {
      FrameStep s;
      s.d_features = d_features + f * fstride;
      s.d_lpc_frame = b->d_lpc + (size_t)(f - c0) * b->B * NLPC; /* computed above */
      s.d_pcm = d_pcm + (size_t)f * b->B * N;
      s.N = N;
      s.ovl = ovl ? f : -1;
      if (launch_frame_step(b, s)) return -1;
    }
  }
  return 0;
}

}  // extern "C"
