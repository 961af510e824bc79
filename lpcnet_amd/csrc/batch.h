/*
 * batch.h -- what engine.cpp (the batch), synth_steps.cpp (its synthesis and
 * decode calls), dropin.cpp (the drop-in handles over them), side_calls.cpp
 * (the PLC, feature, Burg, encoder, RDO-VAE and LPC calls beside synthesis)
 * and conceal_calls.cpp (the concealment machine over all of them) share:
 * struct LPCNetBatch and the buffer groups of the side calls, all of whose
 * device memory, streams and events are held by device_mem.h's owners (so
 * `delete b` releases them); the stream-state helpers, the timed regions, the
 * partial-batch steps a StatePool runs on its work batch and the machine on
 * its work states, and what a batch's load and reset call of side_calls.cpp
 * and conceal_calls.cpp.  Internal to those five files.
 */
#ifndef LPCNET_BATCH_H
#define LPCNET_BATCH_H

#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "device_mem.h"
#include "lpcnet_engine.h"
#include "lpcnet_mi355x.h"
#include "model_host.h"
#include "side_kernels.h"
#include "side_tables.h"

/* LPCNetBatch is the C API's type, outside the namespace its fields come from */
using namespace lpcnet_mi355x;

#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess) {                                                                \
      set_err(std::string(#x) + ": " + hipGetErrorString(e_));                            \
      return -1;                                                                           \
    }                                                                                      \
  } while (0)

/* The timed regions: lpcnet_batch_kernel_ms's `which`.  7 is no region and
 * stays refused: callers probe it as the first invalid value. */
enum TimedRegion {
  TIMED_SAMPLE = 0,     /* sample kernel */
  TIMED_FRAME = 1,      /* frame kernel */
  TIMED_PLC = 2,        /* PLC predictor */
  TIMED_FEAT = 3,       /* feature extractor */
  TIMED_ENC = 4,        /* encoder */
  TIMED_ENC_KERNEL = 5, /* the part of the encoder that is enc_kernel.hip */
  TIMED_BURG = 6,       /* Burg analysis (its three launches) */
  TIMED_NONE = 7,
  TIMED_RDOVAE_ENC = 8, /* RDO-VAE encoder */
  TIMED_RDOVAE_DEC = 9, /* RDO-VAE decoder */
  TIMED_REGIONS = 10
};

/* The device buffers of the calls beside synthesis (side_calls.cpp), one
 * value-initialised group per family.  A carved group owns its buffer (base)
 * and keeps the planned pointers as plain members: freeing it is `= {}`.
 * PLC prediction network (plc_kernel.hip): each stream's plc_gru1_state |
 * plc_gru2_state outside StreamState (the synthesis snapshots keep their
 * size) and the host-I/O staging; they and the tables are buffers of their
 * own, owned by LPCNetBatch's plc_bufs (a re-plan of the synthesis tables
 * keeps them). */
struct PlcBufs {
  float *state = nullptr;
  float *in = nullptr, *out = nullptr; /* [B][PLC_IN], [B][NF] */
  unsigned char *act = nullptr;
};
/* feature extractor (feat_kernel.hip): no weights, so nothing here depends
 * on the model; each stream's analysis state, the constant tables and the
 * host-I/O staging, one buffer (base) allocated by the first call that
 * extracts features (feat_ensure) */
struct FeatBufs {
  DevPtr<char> base;
  FeatState *state = nullptr;
  FeatTables *tab = nullptr;
  float *pcm = nullptr; /* [B][FRAME] float or short */
  float *out = nullptr; /* [B][NTF] */
  unsigned char *act = nullptr;
};
/* Burg cepstral analysis (burg_kernel.hip): stateless; its table and the
 * scratch of one call in one buffer, allocated by the first call that runs
 * it (burg_ensure); it shares the extractor's tables and host-I/O staging */
struct BurgBufs {
  DevPtr<char> base;
  BurgTables *tab = nullptr;
  double *c = nullptr; /* [BURG_NC][2 B] */
  float *x = nullptr;  /* [2 NLPC][2 B] */
  float *o = nullptr;  /* [NLPC + 1][2 B] */
};
/* 1.6 kb/s encoder (feat_kernel<true>, enc_kernel.hip), allocated by the
 * first encode call (enc_ensure) in one buffer: each stream's encoder vq_mem
 * (state, beside the extractor's; not the decoder's), the main_pitch table,
 * the scratch of one packet and the host-I/O staging */
struct EncBufs {
  DevPtr<char> base;
  float *vq = nullptr; /* [B][NBANDS] */
  EncTables *tab = nullptr;
  float *xc = nullptr, *fw = nullptr, *feat = nullptr, *lpc = nullptr;
  int *fields = nullptr;
  short *pcm = nullptr;        /* [4][B][FRAME] */
  unsigned char *pk = nullptr; /* [B][8] */
  float *out = nullptr;        /* [4][B][NTF] */
};

/* DRED RDO-VAE (rdovae_kernel.hip): the tables of each usable side, uploaded
 * with the model into buffers of their own (rdovae_bufs: a re-plan of the
 * synthesis tables keeps them), and what the first RDO-VAE call allocates in
 * one zeroed buffer (rdovae_ensure): each stream's encoder state (the three
 * GRU states, the conv memory) and decoder state (the three GRU states),
 * decode_all's scratch state, the concatenation scratch and the host-I/O
 * staging */
struct RdovaeBufs {
  DevPtr<char> base;
  float *enc_state = nullptr, *enc_mem = nullptr; /* [B][nt], [B][(ksize - 1) T] */
  float *dec_state = nullptr, *dec_scratch = nullptr; /* [B][nt] */
  float *cat = nullptr;                           /* [tiles][T max][PLC_TILE] */
  float *in = nullptr, *lat = nullptr, *st = nullptr, *out = nullptr; /* staging */
  unsigned char *act = nullptr;
};

struct ConcealMachine; /* conceal_calls.cpp */

/* ------------------------------------------------------------------------ */
struct LPCNetBatch {
  int device = 0;
  int B = 0;
  /* Declared before every buffer, the streams before the events: members go
   * in reverse order, so `delete b` frees the buffers, then destroys the
   * events, then the streams.  fstream, ev_start, ev_frame and ev_samp are the
   * overlapped multi-frame path's (below), ev_tick the end of a host-I/O tick
   * (spin-polled), tev the timing events handed out since the last reset
   * (taken) and those waiting for reuse (idle). */
  DevStream stream, fstream;
  DevEvent ev_frame[2], ev_samp[2], ev_start, ev_tick;
  EventPool tev;
  /* model */
  bool have_model = false;
  int variant = 0;
  bool sat = false;
  int kernel_mode = 0;   /* 0 auto, 1 lockstep sample_kernel, 4 matrix-core mf_kernel, 5 fp32 fp_kernel */
  ModelConst mc{1.0f, DEFAULT_FEATURES_DELAY, 0}; /* FEATURES_DELAY / LPC_GAMMA / END2END of the model */
  /* rcpps table of the device activations (RCP_ENTRIES, device form t + kRcpBias);
   * rcp_custom: not the default Intel table (lpcnet_batch_set_rcp_table) */
  bool rcp_custom = false;
  std::vector<uint32_t> rcp_dev;
  ModelCaps caps{};      /* what the kernel choice takes from the model (kernel_choice.h) */
  SamplePlan plan{};     /* the batch's sample kernels: plan_sample_kernels, per launch kernel_for_launch */
  bool plan_wide = false; /* the register tables were planned for mfw_kernel (plan class 3) */
  L2Warm ck_warm{};       /* the chunk kernel's re-tiled weights (deferred LPC warms them) */
  std::vector<unsigned char> blob; /* the loaded model's blob: replanned when the kernel choice moves */
  /* The loaded model's host tables (their blob views look into `blob`), kept
   * until the next load replaces them: 12 to 25 MB.  Returning that memory to
   * the system at the end of the load costs the sample kernels of this
   * process about 1 % at 1,024 streams (same box, alternating runs,
   * profiles/r12: 0.4018 against 0.3976 ms per frame step on the skewed
   * model, the parent commit 0.3967); the mechanism below that is not known. */
  std::unique_ptr<HostModel> host;
  int image_bytes = 0;
  LPCNetModelInfo info{};
  DeviceTables model_bufs;
  FrameArgs fa{};
  SampleTables sample{}; /* the sample kernels' model side, device pointers set (load_model) */
  /* streams */
  DevPtr<StreamState> d_state;
  DevPtr<float> d_feat;
  DevPtr<short> d_pcm;
  DevPtr<float> d_lpc;             /* [LPC_CHUNK][B][NLPC] lpc_from_cepstrum of queued frames */
  DevPtr<LpcTables> d_lpc_tab;
  /* overlapped multi-frame path (few streams, free CUs): frame kernel f+1 on
   * fstream beside sample kernel f on stream, outputs double-buffered in
   * d_cond[f & 1] */
  DevPtr<FrameCond> d_cond[2];
  bool ev_samp_used[2] = {false, false};
  hipEvent_t ev_samp_cur[2] = {nullptr, nullptr}; /* the event slot c's reuse waits on */
  /* chunked multi-frame path (batches above OVERLAP_MAX_STREAMS): the frame
   * network of up to LPC_CHUNK frames in one chunk_kernel launch, outputs of
   * frame f in d_chunk[f][B] */
  DevPtr<FrameCond> d_chunk;
  bool chunking = true;
  /* per-frame host-I/O path of large batches (synth_first): one frame's
   * chunk_kernel outputs [B], and pinned staging of the caller's features and
   * PCM (so both copies are asynchronous, behind one synchronisation).
   * The features live in one of two owners, of which h_io_feat / d_io_feat
   * are the views the hot path reads. */
  DevPtr<float> io_feat_dev;     /* host-visible device memory (fine-grained VRAM, large BAR), or */
  PinnedPtr<float> io_feat_host; /* mapped pinned host memory */
  float *h_io_feat = nullptr;
  float *d_io_feat = nullptr; /* h_io_feat's device address */
  bool io_feat_vram = false;  /* h_io_feat is io_feat_dev's */
  PinnedPtr<short> h_io_pcm;
  short *d_io_pcm = nullptr; /* h_io_pcm's device address (mapped) */
  PinnedPtr<float> h_stg_feat; /* pinned staging of the caller's own buffers */
  PinnedPtr<short> h_stg_pcm;
  /* trace */
  bool trace = false;
  DevPtr<float> d_trace_logits; /* both or neither (ensure_trace) */
  DevPtr<int> d_trace_exc;
  float *trace_logits = nullptr; /* what the sample launches write: the two buffers above */
  int *trace_exc = nullptr;      /* (ensure_trace), or null */
  int trace_N = 0;
  /* device -> host status word (pinned, mapped): a kernel that aborts sets
   * STATUS_* bits; every synchronising entry point checks and clears it */
  PinnedPtr<int> h_status;
  int *d_status = nullptr; /* h_status's device address */
  DevPtr<int> d_ck_sync; /* [ceil(B / 16)] arrival counters of the sliced one-frame chunk kernel */
  int spin_limit = FLAG_SPIN_LIMIT_DEFAULT;
  /* 1.6 kb/s decoder (decode_kernel.hip): the model's ceps codebooks (optional
   * blob records), packets and decoded features of up to DEC_MAX_PACKETS
   * packets per stream, the host-I/O path's 4-frame PCM */
  DecodeArgs da{};
  bool has_codebooks = false;
  DevPtr<unsigned char> d_packets;
  DevPtr<float> d_dfeat;
  DevPtr<short> d_dpcm;
  /* PLC prediction network: optional blob records */
  bool plc_ok = false;
  std::string plc_why = "no model loaded"; /* why the PLC calls refuse this batch */
  PlcArgs pa{};
  DeviceTables plc_bufs; /* the tables, then the state and staging plc points into */
  /* DRED RDO-VAE: optional blob records, each side on its own */
  bool rdo_ok[2] = {false, false}; /* encoder, decoder */
  std::string rdo_why[2] = {"no model loaded", "no model loaded"};
  RdovaeNet rdo_net[2] = {};
  int rdo_dims[RDOVAE_DIMS] = {};
  DeviceTables rdovae_bufs;
  RdovaeBufs rdo{};
  /* the buffers of the calls beside synthesis */
  PlcBufs plc{};
  FeatBufs feat{};
  BurgBufs burg{};
  EncBufs enc{};
  /* the concealment machine (lpcnet_batch_conceal_open), null without one */
  ConcealMachine *conceal = nullptr;
  /* diagnostics */
  DevPtr<unsigned long long> d_stamps;
  /* timing */
  int timing = 0;        /* 0 off, 1 sample kernel, 2 sample + frame kernel */
  std::vector<hipEvent_t> ev_pairs[TIMED_REGIONS]; /* per TimedRegion: (start, end) events of tev */
  std::vector<int> ev_frames[TIMED_REGIONS];       /* frames covered by each pair */
  /* lower bound of every stream's frame_count (lpcnet.c:119) before the next
   * frame: the multi-frame sample launches start where no stream can still
   * be inside its first `delay` (FEATURES_DELAY) frames */
  int min_fc = 0;
  void frames_done(int n) { min_fc = min_fc >= 1000 ? min_fc : std::min(min_fc + n, 1000); }
  int set_device() { return hipSetDevice(device) == hipSuccess ? 0 : -1; }
};

namespace lpcnet_mi355x {

/* Work a caller enqueues on b->stream after a step's kernels, before its one
 * synchronisation (the drop-in pool's state scatter). */
using PreSync = std::function<int()>;

/* a stream's state after lpcnet_init / lpcnet_reset_signal; whether a
 * snapshot is one this engine can have produced (set_err when not) */
void host_reset_state(StreamState &s);
void reset_signal(StreamState &s);
bool snapshot_ok(const void *buf);
/* every value in [-2, 2] or NaN: what a GRU recurrence of this engine leaves */
bool gru_state_plausible(const float *v, size_t n);

/* Timed regions (lpcnet_batch_kernel_ms; engine.cpp).  mark: with `on`, take
 * an event and record it on `s` (e = nullptr otherwise).  timed: the pair
 * (e0, e1) covers `frames` frames of region `which` (a TimedRegion); a null
 * event: no pair. */
int mark(LPCNetBatch *b, bool on, hipStream_t s, hipEvent_t &e);
void timed(LPCNetBatch *b, int which, hipEvent_t e0, hipEvent_t e1, int frames);
/* engine.cpp.  ensure_trace: before the sample launches of a call of N samples
 * per frame, the batch's trace buffers (allocated here, both or neither) as
 * the launches' trace targets (b->trace_logits, b->trace_exc), or none.
 * check_status: after a sync of b->stream, report (set_err, -1) and clear a
 * device-side abort. */
int ensure_trace(LPCNetBatch *b, int N);
int check_status(LPCNetBatch *b);

/* One launch on b->stream as a timed region: with `on`, an event before and
 * one after it; with timing off no event is taken and nothing but the launch
 * is queued.  launch() != 0: -1 with `fail` as the error (null: launch has
 * set its own). */
template <class Launch>
int timed_launch(LPCNetBatch *b, int which, bool on, int frames, const char *fail, Launch &&launch)
{
  hipEvent_t e0, e1;
  if (mark(b, on, b->stream, e0)) return -1;
  if (launch()) {
    if (fail) set_err(fail);
    return -1;
  }
  if (mark(b, e0 != nullptr, b->stream, e1)) return -1;
  timed(b, which, e0, e1, frames);
  return 0;
}

/* One step for the first nB streams of a batch, host I/O, `pre` queued
 * behind its kernels (synth_steps.cpp, at each definition).  staged: the caller
 * has queued the features / preload copies on b->stream already. */
int synth_first(LPCNetBatch *b, int nB, const float *features, short *pcm, int N, int preload,
                const PreSync &pre = PreSync(), bool staged = false);
int tail_first(LPCNetBatch *b, int nB, short *pcm, int N, int preload, const PreSync &pre = PreSync());
int frame_first(LPCNetBatch *b, int nB, const float *features, bool keep_cond, const PreSync &pre = PreSync());
int decode_first(LPCNetBatch *b, int nB, const unsigned char *packets, short *pcm, const PreSync &pre = PreSync());
/* The device-I/O siblings of the three steps above: d_features [nB][NF] and
 * d_pcm [nB][N] are device memory, everything is queued on b->stream and
 * nothing is copied to or from the host or waited for.  They run on the nB
 * states st points to (null: the batch's own first nB): the concealment
 * machine's work states, gathered from and scattered to the batch's.  Only
 * a frame network run on the batch's own states counts into min_fc. */
int synth_first_device(LPCNetBatch *b, int nB, const float *d_features, short *d_pcm, int N, int preload, StreamState *st = nullptr);
int tail_first_device(LPCNetBatch *b, int nB, short *d_pcm, int N, int preload, StreamState *st = nullptr);
int frame_first_device(LPCNetBatch *b, int nB, const float *d_features, bool keep_cond, StreamState *st = nullptr);

/* side_calls.cpp.  plc_load: after a successful model load, with its blob's
 * records (optional: a blob without them loads as ever, plc_why says why the
 * PLC calls refuse it); plc_free, feat_free: the PLC tables and state, the
 * feature extractor's buffers. */
void plc_load(LPCNetBatch *b, const std::vector<Arr> &L);
void plc_free(LPCNetBatch *b);
void feat_free(LPCNetBatch *b);
/* rdovae_load, rdovae_free: the same for the RDO-VAE's tables and, freed
 * only, its state and scratch (a new model has other dimensions) */
void rdovae_load(LPCNetBatch *b, const std::vector<Arr> &L);
void rdovae_free(LPCNetBatch *b);
/* side_reset: queue on b->stream the zeroing of the side state the batch
 * holds, of one stream or of all (stream < 0): the predictor's GRU states
 * (SIDE_PLC), the analysis state and the encoder's vq_mem (SIDE_FEAT).  The
 * caller synchronises. */
enum { SIDE_PLC = 1, SIDE_FEAT = 2 };
int side_reset(LPCNetBatch *b, int stream, int parts);
/* the single launches of the side calls on b->stream, each a timed region
 * (TIMED_PLC, TIMED_FEAT, TIMED_BURG), and what they need ready:
 * plc_ready (a model with usable PLC records; set_err otherwise), burg_ensure
 * (the extractor's and the Burg tables and scratch) */
int plc_ready(const LPCNetBatch *b);
int burg_ensure(LPCNetBatch *b);
int plc_launch(LPCNetBatch *b, const float *d_in, float *d_out, const unsigned char *d_active);
int feat_launch(LPCNetBatch *b, const short *d_pcm, const float *d_pcm_f, float *d_features, int row, const unsigned char *d_active,
                int stride = 0);
int burg_launch(LPCNetBatch *b, const short *d_pcm, const float *d_pcm_f, float *d_out, int stride, int fill, float flag,
                const unsigned char *d_active);

/* conceal_calls.cpp.  conceal_free: close the batch's machine, if any (a model
 * load, the batch's destruction).  conceal_reset_streams: queue on b->stream
 * lpcnet_plc_reset's part beyond the synthesis, predictor and analysis state
 * for one stream or all (stream < 0); nothing without a machine. */
void conceal_free(LPCNetBatch *b);
int conceal_reset_streams(LPCNetBatch *b, int stream);

}  // namespace lpcnet_mi355x

#endif
