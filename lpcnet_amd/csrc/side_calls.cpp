/*
 * side_calls.cpp -- the device side of the calls beside synthesis: the PLC
 * prediction network (lpcnet_batch_plc_*), the feature extractor
 * (lpcnet_batch_*features*) and the stand-alone lpcnet_mi355x_device_lpc.
 * Their tables are built host-only in side_tables.cpp; the batch they run on
 * and its timed regions are engine.cpp's (batch.h).  Argument errors are
 * reported before any device call.
 */
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "batch.h"

namespace {

/* rows [B][row] of staging d_rows back to the caller's buffer, after every
 * command queued on b->stream: inactive streams keep their row */
int copy_back_active(LPCNetBatch *b, const float *d_rows, int row, float *out, const unsigned char *active)
{
  const size_t B = (size_t)b->B;
  std::vector<float> tmp(B * row);
  HIPCHK(hipMemcpyAsync(tmp.data(), d_rows, tmp.size() * 4, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  for (size_t s = 0; s < B; s++)
    if (!active || active[s]) memcpy(out + s * row, &tmp[s * row], (size_t)row * 4);
  return 0;
}

}  // namespace

/* ---- PLC prediction network (plc_kernel.hip) ------------------------------ */
namespace lpcnet_mi355x {

void plc_free(LPCNetBatch *b)
{
  for (void *p : b->plc_bufs) (void)hipFree(p);
  b->plc_bufs.clear();
  b->d_plc_state = b->d_plc_in = b->d_plc_out = nullptr;
  b->d_plc_act = nullptr;
  b->plc_ok = false;
  b->pa = PlcArgs{};
}

/* after a successful load_model, with its blob's records: the PLC tables and
 * the per-stream predictor state (zero, as lpcnet_plc_init leaves plc_net) */
void plc_load(LPCNetBatch *b, const std::vector<Arr> &L)
{
  plc_free(b);
  PlcHost P;
  if (plc_parse(L, b->variant, P, true)) {
    b->plc_why = last_err();
    return;
  }
  PlcArgs a{};
  a.nstreams = b->B;
  bool ok = true;
  auto up = [&](const void *src, size_t bytes) -> void * {
    void *p = nullptr;
    if (!ok || hipMalloc(&p, bytes) != hipSuccess) { ok = false; return nullptr; }
    b->plc_bufs.push_back(p);
    if (src ? hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) != hipSuccess : hipMemset(p, 0, bytes) != hipSuccess) ok = false;
    return p;
  };
  for (const ModelUpload &u : plc_uploads(P, a)) {
    const void *p = up(u.src, u.bytes);
    memcpy(u.dst, &p, sizeof(p));
  }
  a.state = b->d_plc_state = (float *)up(nullptr, (size_t)b->B * (a.n1 + a.n2) * 4);
  b->d_plc_in = (float *)up(nullptr, (size_t)b->B * PLC_IN * 4);
  b->d_plc_out = (float *)up(nullptr, (size_t)b->B * NF * 4);
  b->d_plc_act = (unsigned char *)up(nullptr, (size_t)b->B);
  if (!ok) {
    plc_free(b);
    b->plc_why = "PLC: device allocation or upload of the predictor tables failed";
    return;
  }
  b->pa = a;
  b->plc_ok = true;
  b->plc_why.clear();
}

void feat_free(LPCNetBatch *b)
{
  (void)hipFree(b->d_feat_state);
  (void)hipFree(b->d_feat_tab);
  (void)hipFree(b->d_feat_pcm);
  (void)hipFree(b->d_feat_out);
  (void)hipFree(b->d_feat_act);
  b->d_feat_state = nullptr;
  b->d_feat_tab = nullptr;
  b->d_feat_pcm = b->d_feat_out = nullptr;
  b->d_feat_act = nullptr;
}

}  // namespace lpcnet_mi355x

static int plc_ready(const LPCNetBatch *b)
{
  if (!b) { set_err("null batch"); return -1; }
  if (!b->have_model) { set_err("no model loaded"); return -1; }
  if (!b->plc_ok) { set_err(b->plc_why.empty() ? "PLC: no usable PLC records" : b->plc_why); return -1; }
  return 0;
}

/* one predictor launch on the batch's stream (timed as which = 2 when timing is on) */
static int plc_launch(LPCNetBatch *b, const float *d_in, float *d_out, const unsigned char *d_active)
{
  PlcArgs a = b->pa;
  a.in = d_in;
  a.out = d_out;
  a.active = d_active;
  a.rcp = b->fa.rcp;
  a.rcp_hw = b->sa.rcp_hw;
  return timed_launch(b, 2, b->timing != 0, 1, "plc kernel launch failed", [&] { return launch_plc(a, b->stream); });
}

extern "C" {

LPCNET_EXPORT int lpcnet_batch_plc_info(const LPCNetBatch *b, int dims[4])
{
  if (plc_ready(b)) return -1;
  if (!dims) { set_err("bad arguments"); return -1; }
  dims[0] = PLC_IN;
  dims[1] = b->pa.cond;
  dims[2] = b->pa.n1;
  dims[3] = b->pa.n2;
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_plc_predict_device(LPCNetBatch *b, const float *d_in, float *d_out, const unsigned char *d_active)
{
  if (plc_ready(b) || b->set_device()) return -1;
  return plc_launch(b, d_in, d_out, d_active);
}

LPCNET_EXPORT int lpcnet_batch_plc_predict(LPCNetBatch *b, const float *in, float *out, const unsigned char *active)
{
  if (plc_ready(b) || b->set_device()) return -1;
  const size_t B = (size_t)b->B;
  if (in) HIPCHK(hipMemcpyAsync(b->d_plc_in, in, B * PLC_IN * 4, hipMemcpyHostToDevice, b->stream));
  if (active) HIPCHK(hipMemcpyAsync(b->d_plc_act, active, B, hipMemcpyHostToDevice, b->stream));
  if (plc_launch(b, in ? b->d_plc_in : nullptr, out ? b->d_plc_out : nullptr, active ? b->d_plc_act : nullptr)) return -1;
  if (!out) {
    HIPCHK(hipStreamSynchronize(b->stream));
    return 0;
  }
  return copy_back_active(b, b->d_plc_out, NF, out, active);
}

LPCNET_EXPORT int lpcnet_batch_plc_reset(LPCNetBatch *b, int stream)
{
  if (plc_ready(b) || b->set_device()) return -1;
  if (stream < -1 || stream >= b->B) { set_err("no such stream"); return -1; }
  const size_t nt = (size_t)b->pa.n1 + b->pa.n2;
  if (stream < 0) HIPCHK(hipMemsetAsync(b->d_plc_state, 0, (size_t)b->B * nt * 4, b->stream));
  else HIPCHK(hipMemsetAsync(b->d_plc_state + (size_t)stream * nt, 0, nt * 4, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_plc_state_size(const LPCNetBatch *b)
{
  if (plc_ready(b)) return -1;
  return (b->pa.n1 + b->pa.n2) * 4;
}

LPCNET_EXPORT int lpcnet_batch_plc_save_state(LPCNetBatch *b, int stream, void *buf)
{
  if (plc_ready(b) || b->set_device()) return -1;
  if (stream < 0 || stream >= b->B || !buf) { set_err("bad arguments"); return -1; }
  const size_t nt = (size_t)b->pa.n1 + b->pa.n2;
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipMemcpy(buf, b->d_plc_state + (size_t)stream * nt, nt * 4, hipMemcpyDeviceToHost));
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_plc_restore_state(LPCNetBatch *b, int stream, const void *buf)
{
  if (plc_ready(b) || b->set_device()) return -1;
  if (stream < 0 || stream >= b->B || !buf) { set_err("bad arguments"); return -1; }
  const size_t nt = (size_t)b->pa.n1 + b->pa.n2;
  std::vector<float> v(nt);
  memcpy(v.data(), buf, nt * 4);
  if (!gru_state_plausible(v.data(), nt)) {
    set_err("PLC snapshot GRU state outside [-2, 2]: not a state this engine produced");
    return -1;
  }
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipMemcpy(b->d_plc_state + (size_t)stream * nt, buf, nt * 4, hipMemcpyHostToDevice));
  return 0;
}

}  // extern "C"

/* ---- feature extractor (lpcnet_compute_single_frame_features) ------------- */

/* the analysis state, tables and staging of a batch, on its first extraction */
static int feat_ensure(LPCNetBatch *b)
{
  if (b->d_feat_state) return 0;
  const size_t B = (size_t)b->B;
  FeatTables T;
  build_feat_tables(T);
  FeatState *st = nullptr;
  FeatTables *tab = nullptr;
  float *pcm = nullptr, *out = nullptr;
  unsigned char *act = nullptr;
  const bool ok = hipMalloc(&st, sizeof(FeatState) * B) == hipSuccess &&
                  hipMemsetAsync(st, 0, sizeof(FeatState) * B, b->stream) == hipSuccess && /* ordered before the first launch */
                  hipMalloc(&tab, sizeof(T)) == hipSuccess && hipMemcpy(tab, &T, sizeof(T), hipMemcpyHostToDevice) == hipSuccess &&
                  hipMalloc(&pcm, B * FRAME * 4) == hipSuccess && hipMalloc(&out, B * NTF * 4) == hipSuccess &&
                  hipMalloc(&act, B) == hipSuccess;
  if (!ok) {
    (void)hipFree(st);
    (void)hipFree(tab);
    (void)hipFree(pcm);
    (void)hipFree(out);
    (void)hipFree(act);
    set_err("features: device allocation failed");
    return -1;
  }
  b->d_feat_state = st;
  b->d_feat_tab = tab;
  b->d_feat_pcm = pcm;
  b->d_feat_out = out;
  b->d_feat_act = act;
  return 0;
}

/* one extractor launch on the batch's stream (timed as which = 3 when timing is on) */
static int feat_launch(LPCNetBatch *b, const short *d_pcm, const float *d_pcm_f, float *d_features, int row,
                       const unsigned char *d_active)
{
  FeatArgs a{};
  a.nstreams = b->B;
  a.pcm = d_pcm;
  a.pcm_f = d_pcm_f;
  a.features = d_features;
  a.row = row;
  a.active = d_active;
  a.state = b->d_feat_state;
  a.lpc_tab = b->d_lpc_tab;
  a.tab = b->d_feat_tab;
  return timed_launch(b, 3, b->timing != 0, 1, "feature kernel launch failed", [&] { return launch_feat(a, b->stream); });
}

static int feat_host(LPCNetBatch *b, const void *pcm, bool is_float, float *features, const unsigned char *active)
{
  if (!pcm || !features) { set_err("bad arguments"); return -1; }
  if (!b) { set_err("null batch"); return -1; }
  if (b->set_device() || feat_ensure(b)) return -1;
  const size_t B = (size_t)b->B;
  HIPCHK(hipMemcpyAsync(b->d_feat_pcm, pcm, B * FRAME * (is_float ? 4 : 2), hipMemcpyHostToDevice, b->stream));
  if (active) HIPCHK(hipMemcpyAsync(b->d_feat_act, active, B, hipMemcpyHostToDevice, b->stream));
  if (feat_launch(b, is_float ? nullptr : (const short *)b->d_feat_pcm, is_float ? b->d_feat_pcm : nullptr, b->d_feat_out, NTF,
                  active ? b->d_feat_act : nullptr))
    return -1;
  return copy_back_active(b, b->d_feat_out, NTF, features, active);
}

extern "C" {

LPCNET_EXPORT int lpcnet_batch_compute_features(LPCNetBatch *b, const short *pcm, float *features, const unsigned char *active)
{
  return feat_host(b, pcm, false, features, active);
}

LPCNET_EXPORT int lpcnet_batch_compute_features_float(LPCNetBatch *b, const float *pcm, float *features,
                                                      const unsigned char *active)
{
  return feat_host(b, pcm, true, features, active);
}

LPCNET_EXPORT int lpcnet_batch_compute_features_device(LPCNetBatch *b, const short *d_pcm, float *d_features, int row,
                                                       const unsigned char *d_active, int nframes)
{
  if (row != NF && row != NTF) { set_err("features: row must be NB_FEATURES (20) or NB_TOTAL_FEATURES (36)"); return -1; }
  if (nframes < 0) { set_err("features: nframes < 0"); return -1; }
  if (!d_pcm || !d_features) { set_err("bad arguments"); return -1; }
  if (!b) { set_err("null batch"); return -1; }
  if (b->set_device() || feat_ensure(b)) return -1;
  /* the frames of a stream are sequential: one launch per frame, in stream order */
  for (int f = 0; f < nframes; f++)
    if (feat_launch(b, d_pcm + (size_t)f * b->B * FRAME, nullptr, d_features + (size_t)f * b->B * row, row, d_active)) return -1;
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_features_reset(LPCNetBatch *b, int stream)
{
  if (stream < -1) { set_err("no such stream"); return -1; }
  if (!b) { set_err("null batch"); return -1; }
  if (stream >= b->B) { set_err("no such stream"); return -1; }
  if (!b->d_feat_state) return 0; /* never used: a first use starts from the reset state */
  if (b->set_device()) return -1;
  if (stream < 0) HIPCHK(hipMemsetAsync(b->d_feat_state, 0, sizeof(FeatState) * (size_t)b->B, b->stream));
  else HIPCHK(hipMemsetAsync(b->d_feat_state + stream, 0, sizeof(FeatState), b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_features_state_size(const LPCNetBatch *) { return (int)sizeof(FeatState); }

LPCNET_EXPORT int lpcnet_batch_features_save_state(LPCNetBatch *b, int stream, void *buf)
{
  if (stream < 0 || !buf) { set_err(stream < 0 ? "no such stream" : "bad arguments"); return -1; }
  if (!b) { set_err("null batch"); return -1; }
  if (stream >= b->B) { set_err("no such stream"); return -1; }
  if (b->set_device() || feat_ensure(b)) return -1;
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipMemcpy(buf, b->d_feat_state + stream, sizeof(FeatState), hipMemcpyDeviceToHost));
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_features_restore_state(LPCNetBatch *b, int stream, const void *buf)
{
  if (stream < 0 || !buf) { set_err(stream < 0 ? "no such stream" : "bad arguments"); return -1; }
  /* the kernel indexes its Viterbi rows with best_i */
  FeatState s;
  memcpy(&s, buf, sizeof(s));
  if (s.best_i < 0 || s.best_i >= PITCH_STATES) { set_err("features snapshot: best_i outside [0, 224): not a state this engine produced"); return -1; }
  if (!b) { set_err("null batch"); return -1; }
  if (stream >= b->B) { set_err("no such stream"); return -1; }
  if (b->set_device() || feat_ensure(b)) return -1;
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipMemcpy(b->d_feat_state + stream, &s, sizeof(s), hipMemcpyHostToDevice));
  return 0;
}

/* ---- lpc_from_cepstrum on its own (lpc_kernel.hip) ------------------------ */
LPCNET_EXPORT int lpcnet_mi355x_device_lpc(int device, const float *cepstra, float *lpc, int n)
{
  if (n < 0 || (n > 0 && (!cepstra || !lpc))) { set_err("bad arguments"); return -1; }
  if (n == 0) return 0;
  if (hipSetDevice(device) != hipSuccess) { set_err("hipSetDevice failed"); return -1; }
  LpcTables T;
  build_lpc_tables(T);
  float *dc = nullptr, *dl = nullptr;
  LpcTables *dt = nullptr;
  int rc = -1;
  if (hipMalloc(&dc, sizeof(float) * NF * (size_t)n) == hipSuccess && hipMalloc(&dl, sizeof(float) * NLPC * (size_t)n) == hipSuccess &&
      hipMalloc(&dt, sizeof(T)) == hipSuccess && hipMemcpy(dt, &T, sizeof(T), hipMemcpyHostToDevice) == hipSuccess) {
    /* cepstra arrive as [n][NLPC+2] (18 bands); the kernel reads [n][NF] */
    std::vector<float> f((size_t)NF * n, 0.f);
    for (int i = 0; i < n; i++) memcpy(&f[(size_t)i * NF], cepstra + (size_t)i * LPC_NBANDS, sizeof(float) * LPC_NBANDS);
    if (hipMemcpy(dc, f.data(), f.size() * 4, hipMemcpyHostToDevice) == hipSuccess && launch_lpc(dc, dl, n, dt, nullptr) == 0 &&
        hipMemcpy(lpc, dl, sizeof(float) * NLPC * (size_t)n, hipMemcpyDeviceToHost) == hipSuccess)
      rc = 0;
  }
  if (rc) set_err("device LPC failed");
  (void)hipFree(dc);
  (void)hipFree(dl);
  (void)hipFree(dt);
  return rc;
}

}  // extern "C"
