/*
 * engine.cpp -- the batch of the MI355X LPCNet synthesis engine: its
 * lifecycle, model, setters, stream state and diagnostics (lpcnet_batch_*
 * beside synthesis, and the host-only model checks) declared in
 * include/lpcnet_mi355x.h.  The synthesis and decode calls and the launches
 * under them are synth_steps.cpp.  The drop-in single-stream API of
 * include/lpcnet.h is dropin.cpp, over the partial-batch steps declared in
 * batch.h.  The calls beside synthesis -- the PLC predictor, the feature
 * extractor, the Burg analysis, the encoder, the RDO-VAE and
 * lpcnet_mi355x_device_lpc -- are side_calls.cpp, which also loads and frees
 * their tables (plc_load, rdovae_load, called from a model load here); their
 * host-built tables are side_tables.cpp (host-only).  This file lends them
 * its timed regions (batch.h).  Every buffer, stream and event of a batch is
 * held by an owner of device_mem.h, whose HIP backend is device_mem.cpp: no
 * file but that one allocates or frees (the public allocator
 * lpcnet_batch_device_alloc / _free below aside).
 *
 * Responsibilities
 *  - upload of a parsed, validated and re-tiled weight blob (model_host.cpp:
 *    blob -> HostModel; mf_plan.cpp: the GRU_A planner and register tables
 *    of the matrix-core kernels; both host-only) and its commit to a batch;
 *  - the batch's plan of sample kernels (kernel_choice.cpp, host-only) after
 *    a load or a change of the kernel mode or the rcpps table;
 *  - per-stream device state (lpcnet_private.h:28-48) and reset semantics
 *    (lpcnet.c:174-182);
 *  - timed regions, stamps, the trace and the device status word.
 * Compile with -ffp-contract=off, as every translation unit.
 */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cstddef>
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
  b->model_bufs.clear();
  b->have_model = false;
  b->ck_warm = L2Warm{};
}

/* what the kernel choice (kernel_choice.cpp) takes from a host model, and
 * the kernels' dynamic LDS for it */
ModelCaps model_caps(const HostModel &h)
{
  ModelCaps c;
  c.fp_ok = h.fp_ok;
  c.mf_ok = h.mf_ok;
  c.mf_split = h.sample.form.mf_split != 0;
  c.mfw_split = h.sample.form.mfw_split != 0;
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
  b->sample.form.rcp_hw = b->fa.rcp_hw = b->plan.rcp_hw;
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
int upload_model(const HostModel &host, ModelArgs &args, DeviceTables &bufs)
{
  if (bufs.upload(model_uploads(host, args))) {
    set_err("device upload failed");
    return -1;
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
  DeviceTables bufs;
  if (upload_model(host, args, bufs)) return -1;
  if (!host.bounds_note.empty()) fputs(host.bounds_note.c_str(), stderr);
  /* Nothing in *b (a fresh load's freed buffers aside) has changed up to
   * here, and nothing below can fail: every check passed and the last upload
   * succeeded. */
  b->model_bufs = std::move(bufs); /* frees a replan's previous tables */
  b->sample = args.sample;
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

/* Entry 0 of a model digest: the sample kernels' scalars of every family in
 * the one byte layout tests/golden/model_digests.json was recorded with --
 * the launch fields zero, a null pointer where a table's address goes.  A
 * fixture of this layout compares every scalar a load computes with the
 * commit that recorded it, however the kernels' arguments are grouped. */
struct DigestScalars {
  void *st; int delay; void *cond; int nstreams, N, nframes; void *pcm; int preload;
  void *emb[3], *ga_par, *ga_wsum, *gb_par, *gb_wsum, *image;
  int image_bytes, image_lds_bytes;
  int ga_K[SAMPLE_WAVES][3], ga_woff[SAMPLE_WAVES][3], ga_coff[SAMPLE_WAVES][3];
  int gb_nb[GB_ROWS / 8], gb_woff[GB_ROWS / 8], gb_coff[GB_ROWS / 8], gb_rec_off;
  int ga_K4[SAMPLE_WAVES][3], ga_qoff[SAMPLE_WAVES][3], gb_qoff[GB_ROWS / 8];
  void *mf, *mf_unit; float mf_zr_bound, mf_h_bound; int fc_fin; void *mf_emb[3];
  int mf_nzr[SAMPLE_WAVES], mf_nh[SAMPLE_WAVES], mf_split, mf_nfzr[SAMPLE_WAVES], mf_nfh[SAMPLE_WAVES]; void *mf_frow;
  int mfw_split; void *mfw_tab, *mfw_frow, *mfw_unit, *mfw_emb[3];
  int mfw_nzr[MFW_TAB_WAVES], mfw_nh[MFW_TAB_WAVES]; void *mf_gb;
  void *fp_zr, *fp_h, *fp_gb, *fp_off; int fp_nzr[SAMPLE_WAVES], fp_nh[SAMPLE_WAVES];
  int fp_long, fpl_kz, fpl_kh; void *fpl_zr, *fpl_h, *fpl_off;
  void *ga_wf, *gb_wf, *gb_recf;
  void *stamps, *trace_logits, *trace_exc; int rcp_hw; void *status; int spin_limit;
};

uint64_t digest_scalars(const SampleTables &t)
{
  DigestScalars d;
  memset(&d, 0, sizeof(d));
#define COPY(part, m) memcpy(&d.m, &t.part.m, sizeof(d.m)); static_assert(sizeof(d.m) == sizeof(t.part.m), #m)
  COPY(lockstep, image_bytes); COPY(lockstep, image_lds_bytes);
  COPY(lockstep, ga_K); COPY(lockstep, ga_woff); COPY(lockstep, ga_coff);
  COPY(lockstep, gb_nb); COPY(lockstep, gb_woff); COPY(lockstep, gb_coff); COPY(lockstep, gb_rec_off);
  COPY(lockstep, ga_K4); COPY(lockstep, ga_qoff); COPY(lockstep, gb_qoff);
  COPY(mf, mf_zr_bound); COPY(mf, mf_h_bound); COPY(mf, fc_fin);
  COPY(mf, mf_nzr); COPY(mf, mf_nh); COPY(mf, mf_nfzr); COPY(mf, mf_nfh);
  COPY(mfw, mfw_nzr); COPY(mfw, mfw_nh);
  COPY(fp, fp_nzr); COPY(fp, fp_nh); COPY(fp, fpl_kz); COPY(fp, fpl_kh);
  COPY(form, mf_split); COPY(form, mfw_split); COPY(form, fp_long); COPY(form, rcp_hw);
#undef COPY
  return fnv1a64(&d, sizeof(d));
}

}  // namespace

/* Before the sample launches of a call (batch.h): the batch's trace buffers
 * as its sample launches' trace targets, or none. */
int lpcnet_mi355x::ensure_trace(LPCNetBatch *b, int N)
{
  if (!b->trace) {
    b->trace_logits = nullptr;
    b->trace_exc = nullptr;
    return 0;
  }
  if (!b->d_trace_logits) {
    /* both or neither: a batch never holds one without the other */
    DevPtr<float> logits;
    DevPtr<int> exc;
    if (logits.alloc((size_t)b->B * FRAME * 8) || exc.alloc((size_t)b->B * FRAME)) return -1;
    b->d_trace_logits = std::move(logits);
    b->d_trace_exc = std::move(exc);
  }
  b->trace_logits = b->d_trace_logits;
  b->trace_exc = b->d_trace_exc;
  b->trace_N = N;
  return 0;
}

/* ---- timed regions (lpcnet_batch_kernel_ms; batch.h) ---------------------- */
/* mark: with `on`, take an event and record it on `s` (e = nullptr
 * otherwise: with timing off there are no events at all).  The event belongs
 * to tev.taken from the moment it is taken, so a failing call leaks nothing.
 * timed: the pair (e0, e1) covers `frames` frames of region `which` (a
 * TimedRegion, batch.h). */
int lpcnet_mi355x::mark(LPCNetBatch *b, bool on, hipStream_t s, hipEvent_t &e)
{
  e = nullptr;
  if (!on) return 0;
  e = b->tev.take();
  if (!e) { set_err("hipEventCreate failed"); return -1; }
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

/* After a sync of b->stream: report (and clear) a device-side abort. */
int lpcnet_mi355x::check_status(LPCNetBatch *b)
{
  int *const word = b->h_status;
  const int st = __atomic_load_n(word, __ATOMIC_ACQUIRE);
  if (st == 0) return 0;
  __atomic_store_n(word, 0, __ATOMIC_RELEASE);
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
  const size_t nB = (size_t)nb_streams;
  ok = ok && b->stream.create() == 0;
  ok = ok && b->d_state.alloc(nB) == 0;
  ok = ok && b->d_feat.alloc(NF * nB) == 0;
  ok = ok && b->d_pcm.alloc(FRAME * nB) == 0;
  ok = ok && b->h_status.alloc(64 / sizeof(int), true) == 0;
  ok = ok && hipHostGetDevicePointer((void **)&b->d_status, b->h_status, 0) == hipSuccess;
  if (ok) *b->h_status = 0;
  ok = ok && b->d_lpc.alloc(NLPC * nB * LPC_CHUNK) == 0;
  ok = ok && b->d_ck_sync.alloc((nB + 15) / 16) == 0;
  ok = ok && hipMemset(b->d_ck_sync, 0, sizeof(int) * ((nB + 15) / 16)) == hipSuccess;
  ok = ok && b->d_lpc_tab.alloc(1) == 0;
  /* d_chunk (the chunked path's frame outputs, LPC_CHUNK x 4.9 KB per
   * stream) is allocated by the first call that takes that path */
  if (ok) {
    LpcTables T;
    build_lpc_tables(T);
    ok = hipMemcpy(b->d_lpc_tab, &T, sizeof(T), hipMemcpyHostToDevice) == hipSuccess;
  }
  if (ok && nb_streams <= OVERLAP_MAX_STREAMS) {
    ok = ok && b->fstream.create() == 0;
    ok = ok && b->ev_start.create(false) == 0;
    for (int i = 0; i < 2 && ok; i++) {
      ok = ok && b->d_cond[i].alloc(nB) == 0;
      ok = ok && b->ev_frame[i].create(false) == 0;
      ok = ok && b->ev_samp[i].create(false) == 0;
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
  /* the device is current: the owners free the buffers, then the events, then the streams */
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
    rdovae_load(b, b->host->records);
  } else if (!b->have_model) {
    plc_free(b);
    b->plc_why = "no model loaded";
    rdovae_free(b);
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
  HIPCHK(hipMemcpy((unsigned char *)b->sample.model.image + IMG_RCP, dev.data(), RCP_ENTRIES * 4, hipMemcpyHostToDevice));
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
  return rows_save({{b->d_state, sizeof(StreamState)}}, stream, buf, b->stream);
}

LPCNET_EXPORT int lpcnet_batch_restore_state(LPCNetBatch *b, int stream, const void *buf)
{
  if (!b || stream < 0 || stream >= b->B || !buf || b->set_device()) return -1;
  if (!snapshot_ok(buf)) return -1;
  if (rows_restore({{b->d_state, sizeof(StreamState)}}, stream, buf, b->stream)) return -1;
  int fc;
  memcpy(&fc, (const unsigned char *)buf + offsetof(StreamState, frame_count), sizeof(fc));
  b->min_fc = std::min(b->min_fc, fc);
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
  b->tev.recycle();
  b->timing = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
}

LPCNET_EXPORT double lpcnet_batch_kernel_ms(LPCNetBatch *b, int which, int *launches)
{
  if (!b || which < 0 || which >= TIMED_REGIONS || which == TIMED_NONE) return -1;
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
  if (!b || which < 0 || which >= TIMED_REGIONS || which == TIMED_NONE) return -1;
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
  b->d_stamps.reset();
  if (enable) {
    /* sample kernel [groups][STAMP_WAVES][16] (enough for any S), then the
     * frame kernel [B / FRAME_STREAMS][16] */
    size_t n = (size_t)b->B * STAMP_WAVES * 16 + (size_t)(frame_groups(b->B) + 1) * 16;
    if (b->d_stamps.alloc(n)) return -1;
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

/* fixed order: the sample kernels' scalars, the MODEL_TABLES upload entries (0:
 * not part of this model), ck_rep, the kernel-choice scalars, the work numbers */
LPCNET_EXPORT int lpcnet_mi355x_model_digest(const unsigned char *data, int len, int streams, int cus, int wide, uint64_t *out,
                                             int cap)
{
  if (!out || cap < MODEL_TABLES + 4 || streams < 1) { set_err("bad arguments"); return -1; }
  HostModel h;
  if (build_host_model(data, len, build_opts(streams, wide < 0 ? wide_now(streams, 0, false, cus) : wide != 0), h)) return -1;
  ModelArgs args;
  int n = 0;
  out[n++] = digest_scalars(h.sample);
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
