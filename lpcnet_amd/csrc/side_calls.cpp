/*
 * side_calls.cpp -- the device side of the calls beside synthesis: the PLC
 * prediction network (lpcnet_batch_plc_*), the feature extractor
 * (lpcnet_batch_*features*), the Burg analysis, the predictor's input rows
 * and the good-packet step (lpcnet_batch_burg_cepstrum*, _plc_rows_device,
 * _plc_update*), the 1.6 kb/s encoder (lpcnet_batch_encode*), the DRED
 * RDO-VAE (lpcnet_batch_rdovae_*) and the stand-alone
 * lpcnet_mi355x_device_lpc.
 * Their tables are built host-only in side_tables.cpp and uploaded here
 * with a model load (plc_load, rdovae_load); the lazily allocated buffers of
 * each family are carved groups that own their memory (batch.h,
 * device_mem.h), and every reset, save and restore of per-stream state is a
 * list of StateRows.  The batch they run on and its timed regions are
 * engine.cpp's (batch.h).  Argument errors are reported before any device
 * call.
 */
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "batch.h"

namespace {

/* rows [B] of `row` bytes of staging d_rows back to the caller's buffer, after
 * every command queued on b->stream: inactive streams keep their row */
int copy_back_active(LPCNetBatch *b, const void *d_rows, size_t row, void *out, const unsigned char *active)
{
  const size_t B = (size_t)b->B;
  std::vector<char> tmp(B * row);
  HIPCHK(hipMemcpyAsync(tmp.data(), d_rows, tmp.size(), hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  for (size_t s = 0; s < B; s++)
    if (!active || active[s]) memcpy((char *)out + s * row, &tmp[s * row], row);
  return 0;
}

/* the per-stream state of each family as rows (device_mem.h): the
 * predictor's GRU states, the analysis state, the encoder's vq_mem */
StateRows plc_rows_of(const LPCNetBatch *b) { return {b->plc.state, ((size_t)b->pa.n1 + b->pa.n2) * 4}; }
StateRows feat_rows_of(const LPCNetBatch *b) { return {b->feat.state, sizeof(FeatState)}; }
StateRows vq_rows_of(const LPCNetBatch *b) { return {b->enc.vq, NBANDS * 4}; }

}  // namespace

/* ---- PLC prediction network (plc_kernel.hip) ------------------------------ */
namespace lpcnet_mi355x {

void plc_free(LPCNetBatch *b)
{
  b->plc_bufs.clear();
  b->plc = {};
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
  DeviceTables &t = b->plc_bufs;
  bool ok = t.upload(plc_uploads(P, a)) == 0;
  ok = ok && (a.state = b->plc.state = (float *)t.zeroed((size_t)b->B * (a.n1 + a.n2) * 4));
  ok = ok && (b->plc.in = (float *)t.zeroed((size_t)b->B * PLC_IN * 4));
  ok = ok && (b->plc.out = (float *)t.zeroed((size_t)b->B * NF * 4));
  ok = ok && (b->plc.act = (unsigned char *)t.zeroed((size_t)b->B));
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
  b->feat = {};
  b->burg = {};
  b->enc = {};
}

int side_reset(LPCNetBatch *b, int stream, int parts)
{
  std::vector<StateRows> rows;
  if ((parts & SIDE_PLC) && b->plc_ok) rows.push_back(plc_rows_of(b));
  if ((parts & SIDE_FEAT) && b->feat.state) {
    rows.push_back(feat_rows_of(b));
    if (b->enc.vq) rows.push_back(vq_rows_of(b));
  }
  return rows_zero(rows, stream, b->B, b->stream);
}

}  // namespace lpcnet_mi355x

int lpcnet_mi355x::plc_ready(const LPCNetBatch *b)
{
  if (!b) { set_err("null batch"); return -1; }
  if (!b->have_model) { set_err("no model loaded"); return -1; }
  if (!b->plc_ok) { set_err(b->plc_why.empty() ? "PLC: no usable PLC records" : b->plc_why); return -1; }
  return 0;
}

/* one predictor launch on the batch's stream (timed as TIMED_PLC when timing is on) */
int lpcnet_mi355x::plc_launch(LPCNetBatch *b, const float *d_in, float *d_out, const unsigned char *d_active)
{
  PlcArgs a = b->pa;
  a.in = d_in;
  a.out = d_out;
  a.active = d_active;
  a.rcp = b->fa.rcp;
  a.rcp_hw = b->sample.form.rcp_hw;
  return timed_launch(b, TIMED_PLC, b->timing != 0, 1, "plc kernel launch failed", [&] { return launch_plc(a, b->stream); });
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
  if (in) HIPCHK(hipMemcpyAsync(b->plc.in, in, B * PLC_IN * 4, hipMemcpyHostToDevice, b->stream));
  if (active) HIPCHK(hipMemcpyAsync(b->plc.act, active, B, hipMemcpyHostToDevice, b->stream));
  if (plc_launch(b, in ? b->plc.in : nullptr, out ? b->plc.out : nullptr, active ? b->plc.act : nullptr)) return -1;
  if (!out) {
    HIPCHK(hipStreamSynchronize(b->stream));
    return 0;
  }
  return copy_back_active(b, b->plc.out, NF * 4, out, active);
}

LPCNET_EXPORT int lpcnet_batch_plc_reset(LPCNetBatch *b, int stream)
{
  if (plc_ready(b) || b->set_device()) return -1;
  if (stream < -1 || stream >= b->B) { set_err("no such stream"); return -1; }
  if (side_reset(b, stream, SIDE_PLC)) return -1;
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
  return rows_save({plc_rows_of(b)}, stream, buf, b->stream);
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
  return rows_restore({plc_rows_of(b)}, stream, buf, b->stream);
}

}  // extern "C"

/* ---- feature extractor (lpcnet_compute_single_frame_features) ------------- */

/* the analysis state, tables and staging of a batch, on its first extraction */
static int feat_ensure(LPCNetBatch *b)
{
  if (b->feat.base) return 0;
  const size_t B = (size_t)b->B;
  FeatBufs f{};
  Carver c;
  c.add(f.state, B);
  c.add(f.tab, 1);
  c.add(f.pcm, B * FRAME);
  c.add(f.out, B * NTF);
  c.add(f.act, B);
  FeatTables T;
  build_feat_tables(T);
  f.base = c.alloc();
  if (!f.base || hipMemsetAsync(f.state, 0, sizeof(FeatState) * B, b->stream) != hipSuccess || /* ordered before the first launch */
      hipMemcpy(f.tab, &T, sizeof(T), hipMemcpyHostToDevice) != hipSuccess) {
    set_err("features: device allocation failed");
    return -1;
  }
  b->feat = std::move(f);
  return 0;
}

/* the caller's PCM (or what it was rearranged to) into d_dst and its active
 * mask into the extractor's staging, queued on b->stream; d_active: the mask
 * the launches take */
static int stage_in(LPCNetBatch *b, void *d_dst, const void *src, size_t bytes, const unsigned char *active,
                    const unsigned char *&d_active)
{
  HIPCHK(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, b->stream));
  if (active) HIPCHK(hipMemcpyAsync(b->feat.act, active, (size_t)b->B, hipMemcpyHostToDevice, b->stream));
  d_active = active ? b->feat.act : nullptr;
  return 0;
}

/* the extractor's arguments on a batch: one frame of d_pcm (short) or d_pcm_f
 * into rows of `row` values, `stride` apart */
static FeatArgs feat_args(const LPCNetBatch *b, const short *d_pcm, const float *d_pcm_f, float *d_features, int row, int stride,
                          const unsigned char *d_active)
{
  FeatArgs a{};
  a.nstreams = b->B;
  a.pcm = d_pcm;
  a.pcm_f = d_pcm_f;
  a.features = d_features;
  a.row = row;
  a.stride = stride;
  a.active = d_active;
  a.state = b->feat.state;
  a.lpc_tab = b->d_lpc_tab;
  a.tab = b->feat.tab;
  return a;
}

/* one extractor launch on the batch's stream (timed as TIMED_FEAT when timing is on) */
int lpcnet_mi355x::feat_launch(LPCNetBatch *b, const short *d_pcm, const float *d_pcm_f, float *d_features, int row,
                                const unsigned char *d_active, int stride)
{
  /* stride 0: the dense [B][row] of every call but the predictor rows */
  const FeatArgs a = feat_args(b, d_pcm, d_pcm_f, d_features, row, stride ? stride : row, d_active);
  return timed_launch(b, TIMED_FEAT, b->timing != 0, 1, "feature kernel launch failed", [&] { return launch_feat(a, b->stream); });
}

static int feat_host(LPCNetBatch *b, const void *pcm, bool is_float, float *features, const unsigned char *active)
{
  if (!pcm || !features) { set_err("bad arguments"); return -1; }
  if (!b) { set_err("null batch"); return -1; }
  if (b->set_device() || feat_ensure(b)) return -1;
  const unsigned char *d_act;
  if (stage_in(b, b->feat.pcm, pcm, (size_t)b->B * FRAME * (is_float ? 4 : 2), active, d_act)) return -1;
  if (feat_launch(b, is_float ? nullptr : (const short *)b->feat.pcm, is_float ? b->feat.pcm : nullptr, b->feat.out, NTF, d_act)) return -1;
  return copy_back_active(b, b->feat.out, NTF * 4, features, active);
}

/* What the analysis-state snapshot calls (features, encoder) check, in the
 * contract's order: the stream index and the buffer, a restored snapshot's
 * best_i (the kernel indexes its Viterbi rows with it; restore_of names the
 * snapshot in the error), the batch, the stream against it; then the device,
 * the family's buffers (the copy that follows waits for the stream). */
static int snap_ready(LPCNetBatch *b, int stream, const void *buf, const char *restore_of, int (*ensure)(LPCNetBatch *))
{
  if (stream < 0 || !buf) { set_err(stream < 0 ? "no such stream" : "bad arguments"); return -1; }
  if (restore_of) {
    FeatState s;
    memcpy(&s, buf, sizeof(s));
    if (s.best_i < 0 || s.best_i >= PITCH_STATES) {
      set_err(std::string(restore_of) + " snapshot: best_i outside [0, 224): not a state this engine produced");
      return -1;
    }
  }
  if (!b) { set_err("null batch"); return -1; }
  if (stream >= b->B) { set_err("no such stream"); return -1; }
  if (b->set_device() || ensure(b)) return -1;
  return 0;
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
  if (!b->feat.state) return 0; /* never used: a first use starts from the reset state */
  if (b->set_device() || side_reset(b, stream, SIDE_FEAT)) return -1;
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_features_state_size(const LPCNetBatch *) { return (int)sizeof(FeatState); }

LPCNET_EXPORT int lpcnet_batch_features_save_state(LPCNetBatch *b, int stream, void *buf)
{
  if (snap_ready(b, stream, buf, nullptr, feat_ensure)) return -1;
  return rows_save({feat_rows_of(b)}, stream, buf, b->stream);
}

LPCNET_EXPORT int lpcnet_batch_features_restore_state(LPCNetBatch *b, int stream, const void *buf)
{
  if (snap_ready(b, stream, buf, "features", feat_ensure)) return -1;
  return rows_restore({feat_rows_of(b)}, stream, buf, b->stream);
}

}  // extern "C"

/* ---- Burg cepstral analysis, the predictor's input rows (burg_kernel.hip) --- */

static_assert(BURG_N == NTF, "the Burg calls stage their output in the extractor's out");

/* the extractor's tables and staging, and in one buffer the Burg table and
 * the scratch its three stages hand over through, on a batch's first Burg call */
int lpcnet_mi355x::burg_ensure(LPCNetBatch *b)
{
  if (feat_ensure(b)) return -1;
  if (b->burg.base) return 0;
  const size_t n2 = 2 * (size_t)b->B;
  BurgBufs g{};
  Carver c;
  c.add(g.tab, 1);
  c.add(g.c, BURG_NC * n2);
  c.add(g.x, 2 * NLPC * n2);
  c.add(g.o, (NLPC + 1) * n2);
  BurgTables T;
  build_burg_tables(T);
  g.base = c.alloc();
  if (!g.base || hipMemcpy(g.tab, &T, sizeof(T), hipMemcpyHostToDevice) != hipSuccess) {
    set_err("burg: device allocation failed");
    return -1;
  }
  b->burg = std::move(g);
  return 0;
}

/* one Burg analysis (its three launches) on the batch's stream, timed as one region, TIMED_BURG, when timing is on */
int lpcnet_mi355x::burg_launch(LPCNetBatch *b, const short *d_pcm, const float *d_pcm_f, float *d_out, int stride, int fill, float flag,
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
  a.tab = b->feat.tab;
  a.btab = b->burg.tab;
  a.cbuf = b->burg.c;
  a.xbuf = b->burg.x;
  a.obuf = b->burg.o;
  return timed_launch(b, TIMED_BURG, b->timing != 0, 1, "Burg kernel launch failed", [&] { return launch_burg(a, b->stream); });
}

static int burg_host(LPCNetBatch *b, const void *pcm, bool is_float, float *ceps, const unsigned char *active)
{
  if (!pcm || !ceps) { set_err("bad arguments"); return -1; }
  if (!b) { set_err("null batch"); return -1; }
  if (b->set_device() || burg_ensure(b)) return -1;
  const unsigned char *d_act;
  if (stage_in(b, b->feat.pcm, pcm, (size_t)b->B * FRAME * (is_float ? 4 : 2), active, d_act)) return -1;
  if (burg_launch(b, is_float ? nullptr : (const short *)b->feat.pcm, is_float ? b->feat.pcm : nullptr, b->feat.out, BURG_N, 0, 0.f, d_act))
    return -1;
  return copy_back_active(b, b->feat.out, BURG_N * 4, ceps, active);
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
  if (plc_rows(b, d_pcm, b->plc.in, LPCNET_PLC_ROW_BURG | LPCNET_PLC_ROW_FEATURES, 1.f, d_active)) return -1;
  return plc_launch(b, b->plc.in, d_out, d_active);
}

LPCNET_EXPORT int lpcnet_batch_plc_update(LPCNetBatch *b, const short *pcm, float *out, const unsigned char *active)
{
  if (plc_ready(b)) return -1;
  if (!pcm || !out) { set_err("bad arguments"); return -1; }
  if (b->set_device() || burg_ensure(b)) return -1;
  const unsigned char *d_act;
  if (stage_in(b, b->feat.pcm, pcm, (size_t)b->B * FRAME * 2, active, d_act)) return -1;
  if (plc_rows(b, (const short *)b->feat.pcm, b->plc.in, LPCNET_PLC_ROW_BURG | LPCNET_PLC_ROW_FEATURES, 1.f, d_act)) return -1;
  if (plc_launch(b, b->plc.in, b->plc.out, d_act)) return -1;
  return copy_back_active(b, b->plc.out, NF * 4, out, active);
}

}  // extern "C"

/* ---- 1.6 kb/s encoder (lpcnet_encode, lpcnet_compute_features) ------------- */

/* the encoder's vq_mem, table, per-packet scratch and staging of a batch, on
 * its first encode call: one zeroed buffer, every part 256-byte aligned */
static int enc_ensure(LPCNetBatch *b)
{
  if (feat_ensure(b)) return -1;
  if (b->enc.base) return 0;
  const size_t B = (size_t)b->B;
  EncBufs n{};
  Carver c;
  c.add(n.vq, B * NBANDS);
  c.add(n.tab, 1);
  c.add(n.xc, B * 8 * PITCH_MAX);
  c.add(n.fw, B * 8);
  c.add(n.feat, 4 * B * NF);
  c.add(n.lpc, 4 * B * NLPC);
  c.add(n.fields, B * 4);
  c.add(n.pcm, 4 * B * FRAME);
  c.add(n.pk, B * 8);
  c.add(n.out, 4 * B * NTF);
  EncTables T;
  build_enc_tables(T);
  n.base = c.alloc();
  if (!n.base || hipMemsetAsync(n.base, 0, c.size(), b->stream) != hipSuccess ||
      hipMemcpyAsync(n.tab, &T, sizeof(T), hipMemcpyHostToDevice, b->stream) != hipSuccess ||
      hipStreamSynchronize(b->stream) != hipSuccess) { /* T leaves scope */
    set_err("encode: device allocation failed");
    return -1;
  }
  b->enc = std::move(n);
  return 0;
}

/* one packet on the batch's stream: d_pcm [4][B][FRAME]; d_packets [B][8] and
 * d_features [4][B][row] may be null.  Timed as TIMED_ENC (and the launches
 * after the analysis as TIMED_ENC_KERNEL) when timing is on. */
static int enc_packet(LPCNetBatch *b, const short *d_pcm, int quantize, unsigned char *d_packets, float *d_features, int row,
                      const unsigned char *d_active)
{
  const size_t B = (size_t)b->B;
  for (int k = 0; k < 4; k++) {
    FeatArgs a = feat_args(b, d_pcm + k * B * FRAME, nullptr, b->enc.feat + k * B * NF, NF, NF, d_active);
    a.k = k;
    a.xc_out = b->enc.xc;
    a.fw_out = b->enc.fw;
    a.lpc_out = b->enc.lpc + k * B * NLPC;
    if (timed_launch(b, TIMED_ENC, b->timing != 0, 1, "encoder analysis kernel launch failed", [&] { return launch_feat_super(a, b->stream); }))
      return -1;
  }
  EncArgs e{};
  e.nstreams = b->B;
  e.quantize = quantize;
  e.active = d_active;
  e.state = b->feat.state;
  e.vq_mem = b->enc.vq;
  e.xc = b->enc.xc;
  e.fw = b->enc.fw;
  e.feat = b->enc.feat;
  e.fields = b->enc.fields;
  e.lpc = b->enc.lpc;
  e.tab = b->enc.tab;
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
    if (d_features && row == NTF && launch_lpc(b->enc.feat, b->enc.lpc, 4 * b->B, b->d_lpc_tab, b->stream)) {
      set_err("encoder LPC kernel launch failed");
      return -1;
    }
  }
  if (d_features && launch_enc_out(e, b->stream)) { set_err("encoder output kernel launch failed"); return -1; }
  if (mark(b, e0 != nullptr, b->stream, e1)) return -1;
  timed(b, TIMED_ENC, e0, e1, 0);
  timed(b, TIMED_ENC_KERNEL, e0, e1, 4);
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
  const unsigned char *d_act;
  if (stage_in(b, b->enc.pcm, t.data(), t.size() * 2, active, d_act)) return -1;
  if (enc_packet(b, b->enc.pcm, quantize, quantize ? b->enc.pk : nullptr, features ? b->enc.out : nullptr, NTF, d_act)) return -1;
  if (quantize && copy_back_active(b, b->enc.pk, 8, packets, active)) return -1;
  if (features)
    for (int k = 0; k < 4; k++)
      if (copy_back_active(b, b->enc.out + k * B * NTF, NTF * 4, features + k * B * NTF, active)) return -1;
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

/* the features snapshot, then vq_mem */
LPCNET_EXPORT int lpcnet_batch_encode_save_state(LPCNetBatch *b, int stream, void *buf)
{
  if (snap_ready(b, stream, buf, nullptr, enc_ensure)) return -1;
  return rows_save({feat_rows_of(b), vq_rows_of(b)}, stream, buf, b->stream);
}

LPCNET_EXPORT int lpcnet_batch_encode_restore_state(LPCNetBatch *b, int stream, const void *buf)
{
  if (snap_ready(b, stream, buf, "encoder", enc_ensure)) return -1;
  return rows_restore({feat_rows_of(b), vq_rows_of(b)}, stream, buf, b->stream);
}

}  // extern "C"

/* ---- DRED RDO-VAE (rdovae_kernel.hip) -------------------------------------- */
namespace lpcnet_mi355x {

void rdovae_free(LPCNetBatch *b)
{
  b->rdovae_bufs.clear();
  b->rdo = {};
  for (int k = 0; k < 2; k++) {
    b->rdo_ok[k] = false;
    b->rdo_why[k] = "no model loaded";
    b->rdo_net[k] = RdovaeNet{};
  }
  std::fill(b->rdo_dims, b->rdo_dims + RDOVAE_DIMS, 0);
}

/* after a successful load_model, with its blob's records: the tables of each
 * usable side; the state comes with the first call (rdovae_ensure) */
void rdovae_load(LPCNetBatch *b, const std::vector<Arr> &L)
{
  rdovae_free(b);
  RdovaeHost R;
  (void)rdovae_parse(L, b->variant, R, true);
  rdovae_dims_of(R, b->rdo_dims);
  for (int k = 0; k < 2; k++) {
    const RdovaeSide &S = k ? R.dec : R.enc;
    b->rdo_why[k] = S.why;
    if (!S.ok) continue;
    RdovaeNet n;
    const bool ok = b->rdovae_bufs.upload(rdovae_uploads(S, n)) == 0;
    if (ok && rdovae_lds_bytes(n) > 160 * 1024) {
      b->rdo_why[k] = "RDO-VAE: the layer widths need more LDS than a compute unit has";
      continue;
    }
    if (!ok) {
      b->rdo_why[k] = "RDO-VAE: device allocation or upload of the tables failed";
      continue;
    }
    b->rdo_net[k] = n;
    b->rdo_ok[k] = true;
  }
}

}  // namespace lpcnet_mi355x

enum { RDO_ENC = 0, RDO_DEC = 1 };

/* a model with usable records of `side` (set_err otherwise) */
static int rdovae_ready(const LPCNetBatch *b, int side)
{
  if (!b) { set_err("null batch"); return -1; }
  if (!b->have_model) { set_err("no model loaded"); return -1; }
  if (!b->rdo_ok[side]) { set_err(b->rdo_why[side].empty() ? "RDO-VAE: no usable records" : b->rdo_why[side]); return -1; }
  return 0;
}

/* each stream's state (zero, as DRED_rdovae_init_encoder / _decoder leave
 * it), the scratch and the staging of a batch, on its first RDO-VAE call */
static int rdovae_ensure(LPCNetBatch *b)
{
  if (b->rdo.base) return 0;
  const size_t B = (size_t)b->B, tiles = (B + PLC_TILE - 1) / PLC_TILE;
  const RdovaeNet &E = b->rdo_net[RDO_ENC], &D = b->rdo_net[RDO_DEC];
  const int *dm = b->rdo_dims;
  RdovaeBufs r{};
  Carver c;
  if (b->rdo_ok[RDO_ENC]) {
    c.add(r.enc_state, B * E.nt);
    c.add(r.enc_mem, B * (size_t)(E.ksize - 1) * E.T + 1);
  }
  if (b->rdo_ok[RDO_DEC]) {
    c.add(r.dec_state, B * D.nt);
    c.add(r.dec_scratch, B * D.nt);
  }
  c.add(r.cat, tiles * (size_t)std::max(E.T, D.T) * PLC_TILE);
  c.add(r.in, B * 2 * NF);
  c.add(r.lat, B * (size_t)std::max(dm[0], dm[13]));
  c.add(r.st, B * (size_t)std::max(dm[1], dm[14]));
  c.add(r.out, B * RDOVAE_QFRAME);
  c.add(r.act, B);
  r.base = c.alloc();
  if (!r.base || hipMemsetAsync(r.base, 0, c.size(), b->stream) != hipSuccess) { /* ordered before the first launch */
    set_err("RDO-VAE: device allocation failed");
    return -1;
  }
  b->rdo = std::move(r);
  return 0;
}

static RdovaeArgs rdovae_args(const LPCNetBatch *b, int side, const unsigned char *d_active)
{
  RdovaeArgs a{};
  a.net = b->rdo_net[side];
  a.decoder = side;
  a.nstreams = b->B;
  a.active = d_active;
  a.cat = b->rdo.cat;
  a.rcp = b->fa.rcp;
  a.rcp_hw = b->sample.form.rcp_hw;
  return a;
}

/* one encoder launch on the batch's stream (timed as TIMED_RDOVAE_ENC when timing is on) */
static int rdovae_enc_launch(LPCNetBatch *b, const float *d_in, size_t in_stream, size_t in_frame, float *d_latents, float *d_state,
                             const unsigned char *d_active)
{
  RdovaeArgs a = rdovae_args(b, RDO_ENC, d_active);
  a.state = b->rdo.enc_state;
  a.mem = b->rdo.enc_mem;
  a.in = d_in;
  a.in_stream = in_stream;
  a.in_frame = in_frame;
  a.latents = d_latents;
  a.init_state = d_state;
  return timed_launch(b, TIMED_RDOVAE_ENC, b->timing != 0, 1, "RDO-VAE encoder kernel launch failed",
                      [&] { return launch_rdovae(a, b->stream); });
}

/* one decoder launch (TIMED_RDOVAE_DEC): dec_init from d_init when given, then n
 * qframes, on the streams' own state or, with `scratch`, on decode_all's */
static int rdovae_dec_launch(LPCNetBatch *b, const float *d_init, const float *d_lat, float *d_out, int n, bool scratch,
                             const unsigned char *d_active)
{
  RdovaeArgs a = rdovae_args(b, RDO_DEC, d_active);
  a.state = scratch ? b->rdo.dec_scratch : b->rdo.dec_state;
  a.d_init = d_init;
  a.d_lat = d_lat;
  a.d_out = d_out;
  a.nframes = n;
  return timed_launch(b, TIMED_RDOVAE_DEC, b->timing != 0, n, "RDO-VAE decoder kernel launch failed",
                      [&] { return launch_rdovae(a, b->stream); });
}

/* the caller's rows and active mask into the staging, queued on b->stream */
static int rdovae_stage(LPCNetBatch *b, void *d_dst, const void *src, size_t bytes, const unsigned char *active,
                        const unsigned char *&d_active)
{
  if (src) HIPCHK(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, b->stream));
  if (active) HIPCHK(hipMemcpyAsync(b->rdo.act, active, (size_t)b->B, hipMemcpyHostToDevice, b->stream));
  d_active = active ? b->rdo.act : nullptr;
  return 0;
}

/* the floats of one stream's state: which = 1 the encoder's (GRU states, conv
 * memory), 2 the decoder's, 3 both, the encoder's first; -1 (set_err) when a
 * side that is asked for is not usable */
static int rdovae_state_floats(const LPCNetBatch *b, int which, size_t part[3])
{
  if (which < 1 || which > 3) { set_err("RDO-VAE: which must be 1 (encoder), 2 (decoder) or 3 (both)"); return -1; }
  part[0] = part[1] = part[2] = 0;
  if ((which & 1) && rdovae_ready(b, RDO_ENC)) return -1;
  if ((which & 2) && rdovae_ready(b, RDO_DEC)) return -1;
  if (which & 1) {
    part[0] = (size_t)b->rdo_net[RDO_ENC].nt;
    part[1] = (size_t)(b->rdo_net[RDO_ENC].ksize - 1) * b->rdo_net[RDO_ENC].T;
  }
  if (which & 2) part[2] = (size_t)b->rdo_net[RDO_DEC].nt;
  return 0;
}

/* the parts rdovae_state_floats chose, as rows of the batch's buffers */
static std::vector<StateRows> rdovae_rows(const LPCNetBatch *b, const size_t part[3])
{
  float *const base[3] = {b->rdo.enc_state, b->rdo.enc_mem, b->rdo.dec_state};
  std::vector<StateRows> rows;
  for (int k = 0; k < 3; k++)
    if (part[k]) rows.push_back({base[k], part[k] * 4});
  return rows;
}

extern "C" {

LPCNET_EXPORT int lpcnet_batch_rdovae_info(const LPCNetBatch *b, int dims[24])
{
  if (!b) { set_err("null batch"); return -1; }
  if (!b->have_model) { set_err("no model loaded"); return -1; }
  if (!b->rdo_ok[RDO_ENC] && !b->rdo_ok[RDO_DEC]) { set_err(b->rdo_why[RDO_ENC] + "; " + b->rdo_why[RDO_DEC]); return -1; }
  if (!dims) { set_err("bad arguments"); return -1; }
  std::copy(b->rdo_dims, b->rdo_dims + RDOVAE_DIMS, dims);
  for (int k = 0; k < 2; k++) /* a side whose tables did not fit or upload */
    if (!b->rdo_ok[k]) std::fill(dims + (k ? 13 : 0), dims + (k ? RDOVAE_DIMS : 13), 0);
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_rdovae_encode_device(LPCNetBatch *b, const float *d_features, int row, float *d_latents,
                                                    float *d_state, const unsigned char *d_active)
{
  if (row != NF && row != NTF) { set_err("RDO-VAE encode: row must be NB_FEATURES (20) or NB_TOTAL_FEATURES (36)"); return -1; }
  if (rdovae_ready(b, RDO_ENC)) return -1;
  if (!d_features || !d_latents || !d_state) { set_err("bad arguments"); return -1; }
  if (b->set_device() || rdovae_ensure(b)) return -1;
  return rdovae_enc_launch(b, d_features, (size_t)row, (size_t)b->B * row, d_latents, d_state, d_active);
}

LPCNET_EXPORT int lpcnet_batch_rdovae_encode(LPCNetBatch *b, const float *in, float *latents, float *initial_state,
                                             const unsigned char *active)
{
  if (rdovae_ready(b, RDO_ENC)) return -1;
  if (!in || !latents || !initial_state) { set_err("bad arguments"); return -1; }
  if (b->set_device() || rdovae_ensure(b)) return -1;
  const unsigned char *d_act;
  if (rdovae_stage(b, b->rdo.in, in, (size_t)b->B * 2 * NF * 4, active, d_act)) return -1;
  if (rdovae_enc_launch(b, b->rdo.in, 2 * NF, NF, b->rdo.lat, b->rdo.st, d_act)) return -1;
  if (copy_back_active(b, b->rdo.lat, (size_t)b->rdo_dims[0] * 4, latents, active)) return -1;
  return copy_back_active(b, b->rdo.st, (size_t)b->rdo_dims[1] * 4, initial_state, active);
}

LPCNET_EXPORT int lpcnet_batch_rdovae_dec_init_device(LPCNetBatch *b, const float *d_state, const unsigned char *d_active)
{
  if (rdovae_ready(b, RDO_DEC)) return -1;
  if (!d_state) { set_err("bad arguments"); return -1; }
  if (b->set_device() || rdovae_ensure(b)) return -1;
  return rdovae_dec_launch(b, d_state, nullptr, nullptr, 0, false, d_active);
}

LPCNET_EXPORT int lpcnet_batch_rdovae_dec_init(LPCNetBatch *b, const float *state, const unsigned char *active)
{
  if (rdovae_ready(b, RDO_DEC)) return -1;
  if (!state) { set_err("bad arguments"); return -1; }
  if (b->set_device() || rdovae_ensure(b)) return -1;
  const unsigned char *d_act;
  if (rdovae_stage(b, b->rdo.st, state, (size_t)b->B * b->rdo_dims[14] * 4, active, d_act)) return -1;
  if (rdovae_dec_launch(b, b->rdo.st, nullptr, nullptr, 0, false, d_act)) return -1;
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_rdovae_decode_qframe_device(LPCNetBatch *b, const float *d_latents, float *d_qframe,
                                                           const unsigned char *d_active)
{
  if (rdovae_ready(b, RDO_DEC)) return -1;
  if (!d_latents || !d_qframe) { set_err("bad arguments"); return -1; }
  if (b->set_device() || rdovae_ensure(b)) return -1;
  return rdovae_dec_launch(b, nullptr, d_latents, d_qframe, 1, false, d_active);
}

LPCNET_EXPORT int lpcnet_batch_rdovae_decode_qframe(LPCNetBatch *b, const float *latents, float *qframe, const unsigned char *active)
{
  if (rdovae_ready(b, RDO_DEC)) return -1;
  if (!latents || !qframe) { set_err("bad arguments"); return -1; }
  if (b->set_device() || rdovae_ensure(b)) return -1;
  const unsigned char *d_act;
  if (rdovae_stage(b, b->rdo.lat, latents, (size_t)b->B * b->rdo_dims[13] * 4, active, d_act)) return -1;
  if (rdovae_dec_launch(b, nullptr, b->rdo.lat, b->rdo.out, 1, false, d_act)) return -1;
  return copy_back_active(b, b->rdo.out, RDOVAE_QFRAME * 4, qframe, active);
}

LPCNET_EXPORT int lpcnet_batch_rdovae_decode_all_device(LPCNetBatch *b, const float *d_state, const float *d_latents,
                                                        float *d_features, int n, const unsigned char *d_active)
{
  if (n < 0) { set_err("RDO-VAE decode_all: nb_latents < 0"); return -1; }
  if (rdovae_ready(b, RDO_DEC)) return -1;
  if (n == 0) return 0;
  if (!d_state || !d_latents || !d_features) { set_err("bad arguments"); return -1; }
  if (b->set_device() || rdovae_ensure(b)) return -1;
  return rdovae_dec_launch(b, d_state, d_latents, d_features, n, true, d_active);
}

LPCNET_EXPORT int lpcnet_batch_rdovae_decode_all(LPCNetBatch *b, const float *state, const float *latents, float *features, int n,
                                                 const unsigned char *active)
{
  if (n < 0) { set_err("RDO-VAE decode_all: nb_latents < 0"); return -1; }
  if (rdovae_ready(b, RDO_DEC)) return -1;
  if (n == 0) return 0;
  if (!state || !latents || !features) { set_err("bad arguments"); return -1; }
  if (b->set_device() || rdovae_ensure(b)) return -1;
  /* a packet's latents and frames: staging of this call's own size */
  const size_t nl = (size_t)b->B * n * b->rdo_dims[13], no = (size_t)b->B * n * RDOVAE_QFRAME; /* floats */
  DevPtr<float> d_lat, d_out;
  if (d_lat.alloc(nl) || d_out.alloc(no)) {
    set_err("RDO-VAE decode_all: device allocation failed");
    return -1;
  }
  const unsigned char *d_act, *no_mask;
  const int rc = rdovae_stage(b, b->rdo.st, state, (size_t)b->B * b->rdo_dims[14] * 4, active, d_act) ||
                 rdovae_stage(b, d_lat, latents, nl * 4, nullptr, no_mask) ||
                 rdovae_dec_launch(b, b->rdo.st, d_lat, d_out, n, true, d_act) ||
                 copy_back_active(b, d_out, (size_t)n * RDOVAE_QFRAME * 4, features, active);
  /* everything was queued on b->stream, and d_lat and d_out go with this call */
  (void)hipStreamSynchronize(b->stream);
  return rc ? -1 : 0;
}

LPCNET_EXPORT int lpcnet_batch_rdovae_reset(LPCNetBatch *b, int stream, int which)
{
  size_t part[3];
  if (rdovae_state_floats(b, which, part)) return -1;
  if (stream < -1 || stream >= b->B) { set_err("no such stream"); return -1; }
  if (!b->rdo.base) return 0; /* never used: a first use starts from the reset state */
  if (b->set_device()) return -1;
  if (rows_zero(rdovae_rows(b, part), stream, b->B, b->stream)) return -1;
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_rdovae_state_size(const LPCNetBatch *b, int which)
{
  size_t part[3];
  if (rdovae_state_floats(b, which, part)) return -1;
  return (int)((part[0] + part[1] + part[2]) * 4);
}

LPCNET_EXPORT int lpcnet_batch_rdovae_save_state(LPCNetBatch *b, int stream, int which, void *buf)
{
  size_t part[3];
  if (rdovae_state_floats(b, which, part)) return -1;
  if (stream < 0 || stream >= b->B || !buf) { set_err("bad arguments"); return -1; }
  if (b->set_device() || rdovae_ensure(b)) return -1;
  return rows_save(rdovae_rows(b, part), stream, buf, b->stream);
}

LPCNET_EXPORT int lpcnet_batch_rdovae_restore_state(LPCNetBatch *b, int stream, int which, const void *buf)
{
  size_t part[3];
  if (rdovae_state_floats(b, which, part)) return -1;
  if (stream < 0 || stream >= b->B || !buf) { set_err("bad arguments"); return -1; }
  /* the GRU states are what a recurrence of this engine leaves; the conv memory is any floats */
  std::vector<float> v(part[0] + part[1] + part[2]);
  memcpy(v.data(), buf, v.size() * 4);
  if (!gru_state_plausible(v.data(), part[0]) || !gru_state_plausible(v.data() + part[0] + part[1], part[2])) {
    set_err("RDO-VAE snapshot GRU state outside [-2, 2]: not a state this engine produced");
    return -1;
  }
  if (b->set_device() || rdovae_ensure(b)) return -1;
  return rows_restore(rdovae_rows(b, part), stream, v.data(), b->stream);
}

}  // extern "C"

extern "C" {

/* ---- lpc_from_cepstrum on its own (lpc_kernel.hip) ------------------------ */
LPCNET_EXPORT int lpcnet_mi355x_device_lpc(int device, const float *cepstra, float *lpc, int n)
{
  if (n < 0 || (n > 0 && (!cepstra || !lpc))) { set_err("bad arguments"); return -1; }
  if (n == 0) return 0;
  if (hipSetDevice(device) != hipSuccess) { set_err("hipSetDevice failed"); return -1; }
  LpcTables T;
  build_lpc_tables(T);
  DevPtr<float> dc, dl;
  DevPtr<LpcTables> dt;
  int rc = -1;
  if (dc.alloc(NF * (size_t)n) == 0 && dl.alloc(NLPC * (size_t)n) == 0 && dt.alloc(1) == 0 &&
      hipMemcpy(dt, &T, sizeof(T), hipMemcpyHostToDevice) == hipSuccess) {
    /* cepstra arrive as [n][NLPC+2] (18 bands); the kernel reads [n][NF] */
    std::vector<float> f((size_t)NF * n, 0.f);
    for (int i = 0; i < n; i++) memcpy(&f[(size_t)i * NF], cepstra + (size_t)i * LPC_NBANDS, sizeof(float) * LPC_NBANDS);
    if (hipMemcpy(dc, f.data(), f.size() * 4, hipMemcpyHostToDevice) == hipSuccess && launch_lpc(dc, dl, n, dt, nullptr) == 0 &&
        hipMemcpy(lpc, dl, sizeof(float) * NLPC * (size_t)n, hipMemcpyDeviceToHost) == hipSuccess)
      rc = 0;
  }
  if (rc) set_err("device LPC failed"); /* the blocking copy back has waited for the kernel */
  return rc;
}

}  // extern "C"
