/*
 * side_calls.cpp -- the device side of the calls beside synthesis: the PLC
 * prediction network (lpcnet_batch_plc_*), the feature extractor
 * (lpcnet_batch_*features*), the Burg analysis, the predictor's input rows
 * and the good-packet step (lpcnet_batch_burg_cepstrum*, _plc_rows_device,
 * _plc_update*), the 1.6 kb/s encoder (lpcnet_batch_encode*) and the
 * stand-alone lpcnet_mi355x_device_lpc.
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
  (void)hipFree(b->d_enc_base);
  (void)hipFree(b->d_burg_tab);
  b->d_burg_tab = nullptr;
  b->d_burg_c = nullptr;
  b->d_burg_x = b->d_burg_o = nullptr;
  b->d_enc_base = nullptr;
  b->d_enc_vq = b->d_enc_xc = b->d_enc_fw = b->d_enc_feat = b->d_enc_lpc = b->d_enc_out = nullptr;
  b->d_enc_tab = nullptr;
  b->d_enc_fields = nullptr;
  b->d_enc_pcm = nullptr;
  b->d_enc_pk = nullptr;
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
                       const unsigned char *d_active, int stride = 0)
{
  FeatArgs a{};
  a.nstreams = b->B;
  a.pcm = d_pcm;
  a.pcm_f = d_pcm_f;
  a.features = d_features;
  a.row = row;
  a.stride = stride ? stride : row; /* the dense [B][row] of every call but the predictor rows */
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
  if (b->d_enc_vq) {
    if (stream < 0) HIPCHK(hipMemsetAsync(b->d_enc_vq, 0, (size_t)b->B * NBANDS * 4, b->stream));
    else HIPCHK(hipMemsetAsync(b->d_enc_vq + (size_t)stream * NBANDS, 0, NBANDS * 4, b->stream));
  }
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

}  // extern "C"

/* ---- Burg cepstral analysis, the predictor's input rows (burg_kernel.hip) --- */

static_assert(BURG_N == NTF, "the Burg calls stage their output in d_feat_out");

/* the extractor's tables and staging, and in one buffer the Burg table and
 * the scratch its three stages hand over through, on a batch's first Burg call */
static int burg_ensure(LPCNetBatch *b)
{
  if (feat_ensure(b)) return -1;
  if (b->d_burg_tab) return 0;
  const size_t n2 = 2 * (size_t)b->B;
  size_t off = 0;
  auto part = [&](size_t bytes) {
    const size_t o = off;
    off += (bytes + 255) & ~(size_t)255;
    return o;
  };
  const size_t o_tab = part(sizeof(BurgTables)), o_c = part(BURG_NC * n2 * 8), o_x = part(2 * NLPC * n2 * 4), o_o = part((NLPC + 1) * n2 * 4);
  BurgTables T;
  build_burg_tables(T);
  char *base = nullptr;
  if (hipMalloc(&base, off) != hipSuccess || hipMemcpy(base + o_tab, &T, sizeof(T), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(base);
    set_err("burg: device allocation failed");
    return -1;
  }
  b->d_burg_tab = (BurgTables *)(base + o_tab); /* the buffer's start: feat_free frees it */
  b->d_burg_c = (double *)(base + o_c);
  b->d_burg_x = (float *)(base + o_x);
  b->d_burg_o = (float *)(base + o_o);
  return 0;
}

/* one Burg analysis (its three launches) on the batch's stream, timed as one region, which = 6, when timing is on */
static int burg_launch(LPCNetBatch *b, const short *d_pcm, const float *d_pcm_f, float *d_out, int stride, int fill, float flag,
                       const unsigned char *d_active)
{
  BurgArgs a{};
  a.nstreams = b->B;
  a.pcm = d_pcm;
  a.pcm_f = d_pcm_f;
  a.out = d_out;
  a.stride = stride;
  a.fill = fill;
  a.flag = flag;
  a.active = d_active;
  a.lpc_tab = b->d_lpc_tab;
  a.tab = b->d_feat_tab;
  a.btab = b->d_burg_tab;
  a.cbuf = b->d_burg_c;
  a.xbuf = b->d_burg_x;
  a.obuf = b->d_burg_o;
  return timed_launch(b, 6, b->timing != 0, 1, "Burg kernel launch failed", [&] { return launch_burg(a, b->stream); });
}

static int burg_host(LPCNetBatch *b, const void *pcm, bool is_float, float *ceps, const unsigned char *active)
{
  if (!pcm || !ceps) { set_err("bad arguments"); return -1; }
  if (!b) { set_err("null batch"); return -1; }
  if (b->set_device() || burg_ensure(b)) return -1;
  const size_t B = (size_t)b->B;
  HIPCHK(hipMemcpyAsync(b->d_feat_pcm, pcm, B * FRAME * (is_float ? 4 : 2), hipMemcpyHostToDevice, b->stream));
  if (active) HIPCHK(hipMemcpyAsync(b->d_feat_act, active, B, hipMemcpyHostToDevice, b->stream));
  if (burg_launch(b, is_float ? nullptr : (const short *)b->d_feat_pcm, is_float ? b->d_feat_pcm : nullptr, b->d_feat_out, BURG_N, 0, 0.f,
                  active ? b->d_feat_act : nullptr))
    return -1;
  return copy_back_active(b, b->d_feat_out, BURG_N, ceps, active);
}

/* one predictor input row per live stream on the batch's stream, no host
 * round trip: the Burg kernel writes its 36 values, the flag and, without the
 * extractor, the zeros of columns 36..55; the extractor writes its 20 values
 * at column 36 of the 57-wide rows; without the Burg part a fill kernel
 * writes the zeros of columns 0..35 and the flag */
static int plc_rows(LPCNetBatch *b, const short *d_pcm, float *d_rows, int parts, float flag, const unsigned char *d_active)
{
  if (parts & LPCNET_PLC_ROW_BURG) {
    const int fill = BURG_FILL_FLAG | ((parts & LPCNET_PLC_ROW_FEATURES) ? 0 : BURG_FILL_ZERO);
    if (burg_launch(b, d_pcm, nullptr, d_rows, PLC_IN, fill, flag, d_active)) return -1;
  } else if (launch_plc_row_fill(d_rows, flag, d_active, b->B, b->stream)) {
    set_err("predictor row fill kernel launch failed");
    return -1;
  }
  if ((parts & LPCNET_PLC_ROW_FEATURES) && feat_launch(b, d_pcm, nullptr, d_rows + BURG_N, NF, d_active, PLC_IN)) return -1;
  return 0;
}

extern "C" {

LPCNET_EXPORT int lpcnet_batch_burg_cepstrum(LPCNetBatch *b, const short *pcm, float *ceps, const unsigned char *active)
{
  return burg_host(b, pcm, false, ceps, active);
}

LPCNET_EXPORT int lpcnet_batch_burg_cepstrum_float(LPCNetBatch *b, const float *pcm, float *ceps, const unsigned char *active)
{
  return burg_host(b, pcm, true, ceps, active);
}

LPCNET_EXPORT int lpcnet_batch_burg_cepstrum_device(LPCNetBatch *b, const short *d_pcm, float *d_out, int row, int col,
                                                    const unsigned char *d_active, int nframes)
{
  if (col < 0) { set_err("burg: col < 0"); return -1; }
  if (row < col + BURG_N) { set_err("burg: row must be at least col + 36"); return -1; }
  if (nframes < 0) { set_err("burg: nframes < 0"); return -1; }
  if (!d_pcm || !d_out) { set_err("bad arguments"); return -1; }
  if (!b) { set_err("null batch"); return -1; }
  if (b->set_device() || burg_ensure(b)) return -1;
  for (int f = 0; f < nframes; f++)
    if (burg_launch(b, d_pcm + (size_t)f * b->B * FRAME, nullptr, d_out + (size_t)f * b->B * row + col, row, 0, 0.f, d_active)) return -1;
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_plc_rows_device(LPCNetBatch *b, const short *d_pcm, float *d_rows, int parts, float flag,
                                               const unsigned char *d_active)
{
  if (parts < 1 || parts > (LPCNET_PLC_ROW_BURG | LPCNET_PLC_ROW_FEATURES)) {
    set_err("plc rows: parts must be LPCNET_PLC_ROW_BURG, LPCNET_PLC_ROW_FEATURES or both");
    return -1;
  }
  if (!d_pcm || !d_rows) { set_err("bad arguments"); return -1; }
  if (!b) { set_err("null batch"); return -1; }
  if (b->set_device() || burg_ensure(b)) return -1;
  return plc_rows(b, d_pcm, d_rows, parts, flag, d_active);
}

LPCNET_EXPORT int lpcnet_batch_plc_update_device(LPCNetBatch *b, const short *d_pcm, float *d_out, const unsigned char *d_active)
{
  if (plc_ready(b)) return -1;
  if (!d_pcm || !d_out) { set_err("bad arguments"); return -1; }
  if (b->set_device() || burg_ensure(b)) return -1;
  if (plc_rows(b, d_pcm, b->d_plc_in, LPCNET_PLC_ROW_BURG | LPCNET_PLC_ROW_FEATURES, 1.f, d_active)) return -1;
  return plc_launch(b, b->d_plc_in, d_out, d_active);
}

LPCNET_EXPORT int lpcnet_batch_plc_update(LPCNetBatch *b, const short *pcm, float *out, const unsigned char *active)
{
  if (plc_ready(b)) return -1;
  if (!pcm || !out) { set_err("bad arguments"); return -1; }
  if (b->set_device() || burg_ensure(b)) return -1;
  const size_t B = (size_t)b->B;
  HIPCHK(hipMemcpyAsync(b->d_feat_pcm, pcm, B * FRAME * 2, hipMemcpyHostToDevice, b->stream));
  if (active) HIPCHK(hipMemcpyAsync(b->d_feat_act, active, B, hipMemcpyHostToDevice, b->stream));
  const unsigned char *d_act = active ? b->d_feat_act : nullptr;
  if (plc_rows(b, (const short *)b->d_feat_pcm, b->d_plc_in, LPCNET_PLC_ROW_BURG | LPCNET_PLC_ROW_FEATURES, 1.f, d_act)) return -1;
  if (plc_launch(b, b->d_plc_in, b->d_plc_out, d_act)) return -1;
  return copy_back_active(b, b->d_plc_out, NF, out, active);
}

}  // extern "C"

/* ---- 1.6 kb/s encoder (lpcnet_encode, lpcnet_compute_features) ------------- */

/* the encoder's vq_mem, table, per-packet scratch and staging of a batch, on
 * its first encode call: one zeroed buffer, every part 256-byte aligned */
static int enc_ensure(LPCNetBatch *b)
{
  if (feat_ensure(b)) return -1;
  if (b->d_enc_base) return 0;
  const size_t B = (size_t)b->B;
  size_t off = 0;
  auto part = [&](size_t bytes) {
    const size_t o = off;
    off += (bytes + 255) & ~(size_t)255;
    return o;
  };
  const size_t o_vq = part(B * NBANDS * 4), o_tab = part(sizeof(EncTables)), o_xc = part(B * 8 * PITCH_MAX * 4), o_fw = part(B * 8 * 4),
               o_feat = part(4 * B * NF * 4), o_lpc = part(4 * B * NLPC * 4), o_fl = part(B * 4 * 4), o_pcm = part(4 * B * FRAME * 2),
               o_pk = part(B * 8), o_out = part(4 * B * NTF * 4);
  EncTables T;
  build_enc_tables(T);
  char *base = nullptr;
  if (hipMalloc(&base, off) != hipSuccess || hipMemsetAsync(base, 0, off, b->stream) != hipSuccess ||
      hipMemcpyAsync(base + o_tab, &T, sizeof(T), hipMemcpyHostToDevice, b->stream) != hipSuccess ||
      hipStreamSynchronize(b->stream) != hipSuccess) { /* T leaves scope */
    (void)hipFree(base);
    set_err("encode: device allocation failed");
    return -1;
  }
  b->d_enc_base = base;
  b->d_enc_vq = (float *)(base + o_vq);
  b->d_enc_tab = (EncTables *)(base + o_tab);
  b->d_enc_xc = (float *)(base + o_xc);
  b->d_enc_fw = (float *)(base + o_fw);
  b->d_enc_feat = (float *)(base + o_feat);
  b->d_enc_lpc = (float *)(base + o_lpc);
  b->d_enc_fields = (int *)(base + o_fl);
  b->d_enc_pcm = (short *)(base + o_pcm);
  b->d_enc_pk = (unsigned char *)(base + o_pk);
  b->d_enc_out = (float *)(base + o_out);
  return 0;
}

/* one packet on the batch's stream: d_pcm [4][B][FRAME]; d_packets [B][8] and
 * d_features [4][B][row] may be null.  Timed as which = 4 (and the launches
 * after the analysis as 5) when timing is on. */
static int enc_packet(LPCNetBatch *b, const short *d_pcm, int quantize, unsigned char *d_packets, float *d_features, int row,
                      const unsigned char *d_active)
{
  const size_t B = (size_t)b->B;
  for (int k = 0; k < 4; k++) {
    FeatArgs a{};
    a.nstreams = b->B;
    a.pcm = d_pcm + k * B * FRAME;
    a.features = b->d_enc_feat + k * B * NF;
    a.row = NF;
    a.stride = NF;
    a.active = d_active;
    a.state = b->d_feat_state;
    a.lpc_tab = b->d_lpc_tab;
    a.tab = b->d_feat_tab;
    a.k = k;
    a.xc_out = b->d_enc_xc;
    a.fw_out = b->d_enc_fw;
    a.lpc_out = b->d_enc_lpc + k * B * NLPC;
    if (timed_launch(b, 4, b->timing != 0, 1, "encoder analysis kernel launch failed", [&] { return launch_feat_super(a, b->stream); }))
      return -1;
  }
  EncArgs e{};
  e.nstreams = b->B;
  e.quantize = quantize;
  e.active = d_active;
  e.state = b->d_feat_state;
  e.vq_mem = b->d_enc_vq;
  e.xc = b->d_enc_xc;
  e.fw = b->d_enc_fw;
  e.feat = b->d_enc_feat;
  e.fields = b->d_enc_fields;
  e.lpc = b->d_enc_lpc;
  e.tab = b->d_enc_tab;
  if (quantize) {
    e.cb1 = b->da.cb1;
    e.cb2 = b->da.cb2;
    e.cb3 = b->da.cb3;
    e.cbd = b->da.cbd;
    e.pitch = b->da.pitch;
  }
  e.packets = d_packets;
  e.features = d_features;
  e.row = row;
  hipEvent_t e0, e1;
  if (mark(b, b->timing != 0, b->stream, e0)) return -1;
  if (launch_enc_pitch(e, b->stream)) { set_err("encoder pitch kernel launch failed"); return -1; }
  if (quantize) {
    if (launch_enc_vq(e, b->stream)) { set_err("encoder quantiser kernel launch failed"); return -1; }
    /* lpc_from_cepstrum of the four quantised cepstra (lpcnet_enc.c:714-717);
     * unquantised, the analysis has left the same LPC */
    if (d_features && row == NTF && launch_lpc(b->d_enc_feat, b->d_enc_lpc, 4 * b->B, b->d_lpc_tab, b->stream)) {
      set_err("encoder LPC kernel launch failed");
      return -1;
    }
  }
  if (d_features && launch_enc_out(e, b->stream)) { set_err("encoder output kernel launch failed"); return -1; }
  if (mark(b, e0 != nullptr, b->stream, e1)) return -1;
  timed(b, 4, e0, e1, 0);
  timed(b, 5, e0, e1, 4);
  return 0;
}

static int enc_model_ready(const LPCNetBatch *b)
{
  if (!b->have_model) { set_err("lpcnet_encode: no model loaded (the quantiser needs its ceps codebooks)"); return -1; }
  if (!b->has_codebooks) {
    set_err("lpcnet_encode: the model blob carries no ceps_codebook1/2/3 / ceps_codebook_diff4 records");
    return -1;
  }
  return 0;
}

static int enc_host(LPCNetBatch *b, const short *pcm, int quantize, unsigned char *packets, float *features,
                    const unsigned char *active)
{
  if (!pcm || (quantize ? !packets : !features)) { set_err("bad arguments"); return -1; }
  if (!b) { set_err("null batch"); return -1; }
  if (quantize && enc_model_ready(b)) return -1;
  if (b->set_device() || enc_ensure(b)) return -1;
  const size_t B = (size_t)b->B;
  /* [B][640] -> [4][B][160] */
  std::vector<short> t(4 * B * FRAME);
  for (size_t s = 0; s < B; s++)
    for (int k = 0; k < 4; k++) memcpy(&t[(k * B + s) * FRAME], pcm + s * 4 * FRAME + (size_t)k * FRAME, FRAME * 2);
  HIPCHK(hipMemcpyAsync(b->d_enc_pcm, t.data(), t.size() * 2, hipMemcpyHostToDevice, b->stream));
  if (active) HIPCHK(hipMemcpyAsync(b->d_feat_act, active, B, hipMemcpyHostToDevice, b->stream));
  if (enc_packet(b, b->d_enc_pcm, quantize, quantize ? b->d_enc_pk : nullptr, features ? b->d_enc_out : nullptr, NTF,
                 active ? b->d_feat_act : nullptr))
    return -1;
  if (quantize) {
    std::vector<unsigned char> pk(B * 8);
    HIPCHK(hipMemcpyAsync(pk.data(), b->d_enc_pk, pk.size(), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    for (size_t s = 0; s < B; s++)
      if (!active || active[s]) memcpy(packets + s * 8, &pk[s * 8], 8);
  }
  if (features)
    for (int k = 0; k < 4; k++)
      if (copy_back_active(b, b->d_enc_out + k * B * NTF, NTF, features + k * B * NTF, active)) return -1;
  HIPCHK(hipStreamSynchronize(b->stream)); /* t and the staging are free again */
  return 0;
}

extern "C" {

LPCNET_EXPORT int lpcnet_batch_encode(LPCNetBatch *b, const short *pcm, unsigned char *packets, float *features,
                                      const unsigned char *active)
{
  return enc_host(b, pcm, 1, packets, features, active);
}

LPCNET_EXPORT int lpcnet_batch_compute_features4(LPCNetBatch *b, const short *pcm, float *features, const unsigned char *active)
{
  return enc_host(b, pcm, 0, nullptr, features, active);
}

LPCNET_EXPORT int lpcnet_batch_encode_device(LPCNetBatch *b, const short *d_pcm, unsigned char *d_packets, float *d_features,
                                             int row, const unsigned char *d_active, int npackets)
{
  if (row != NF && row != NTF) { set_err("encode: row must be NB_FEATURES (20) or NB_TOTAL_FEATURES (36)"); return -1; }
  if (npackets < 0) { set_err("encode: npackets < 0"); return -1; }
  if (!d_pcm || !d_packets) { set_err("bad arguments"); return -1; }
  if (!b) { set_err("null batch"); return -1; }
  if (enc_model_ready(b)) return -1;
  if (b->set_device() || enc_ensure(b)) return -1;
  const size_t B = (size_t)b->B;
  /* the packets of a stream are sequential: one run of launches per packet */
  for (int p = 0; p < npackets; p++)
    if (enc_packet(b, d_pcm + p * 4 * B * FRAME, 1, d_packets + p * B * 8, d_features ? d_features + p * 4 * B * row : nullptr, row,
                   d_active))
      return -1;
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_encode_state_size(const LPCNetBatch *) { return (int)sizeof(FeatState) + NBANDS * 4; }

LPCNET_EXPORT int lpcnet_batch_encode_save_state(LPCNetBatch *b, int stream, void *buf)
{
  if (stream < 0 || !buf) { set_err(stream < 0 ? "no such stream" : "bad arguments"); return -1; }
  if (!b) { set_err("null batch"); return -1; }
  if (stream >= b->B) { set_err("no such stream"); return -1; }
  if (b->set_device() || enc_ensure(b)) return -1;
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipMemcpy(buf, b->d_feat_state + stream, sizeof(FeatState), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy((char *)buf + sizeof(FeatState), b->d_enc_vq + (size_t)stream * NBANDS, NBANDS * 4, hipMemcpyDeviceToHost));
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_encode_restore_state(LPCNetBatch *b, int stream, const void *buf)
{
  if (stream < 0 || !buf) { set_err(stream < 0 ? "no such stream" : "bad arguments"); return -1; }
  FeatState s;
  memcpy(&s, buf, sizeof(s));
  if (s.best_i < 0 || s.best_i >= PITCH_STATES) { set_err("encoder snapshot: best_i outside [0, 224): not a state this engine produced"); return -1; }
  if (!b) { set_err("null batch"); return -1; }
  if (stream >= b->B) { set_err("no such stream"); return -1; }
  if (b->set_device() || enc_ensure(b)) return -1;
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipMemcpy(b->d_feat_state + stream, &s, sizeof(s), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->d_enc_vq + (size_t)stream * NBANDS, (const char *)buf + sizeof(FeatState), NBANDS * 4, hipMemcpyHostToDevice));
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
