/*
 * model_host.cpp -- blob -> HostModel (see model_host.h).  Compile with
 * -ffp-contract=off: the u-law / logit tables are computed here with the
 * reference's exact expressions.
 */
#include "model_host.h"

#include "device_math.h" /* kTanhFinBound */

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>

namespace lpcnet_mi355x {

namespace {
thread_local std::string g_err;
}
void set_err(const std::string &e) { g_err = e; }
const std::string &last_err() { return g_err; }

const uint32_t kRcpTable[2048] = {
#include "rcp_table_x86.inc"
};

std::vector<uint32_t> default_rcp_dev()
{
  std::vector<uint32_t> t(RCP_ENTRIES);
  for (int i = 0; i < RCP_ENTRIES; i++) t[i] = kRcpTable[i >> (RCP_TABLE_BITS - 11)] + kRcpBias;
  return t;
}

uint64_t fnv1a64(const void *p, size_t n)
{
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char *)p)[i]) * 0x100000001b3ull;
  return h;
}

/* common.h:18-33 + 47-58 */
int host_lin2ulaw(float x)
{
  float scale = 255.f / 32768.f;
  int s = x >= 0 ? 1 : -1;
  x = fabsf(x);
  float y = 1 + scale * x;
  uint32_t bits;
  memcpy(&bits, &y, 4);
  int integer = (int)(bits >> 23) - 127;
  bits -= (uint32_t)integer << 23;
  float m;
  memcpy(&m, &bits, 4);
  float frac = m - 1.5f;
  frac = -0.41445418f + frac * (0.95909232f + frac * (-0.33951290f + frac * 0.16541097f));
  float l2 = 1 + integer + frac;
  float u = (s * (128 * (0.69315f * l2) / 5.5451774445f));
  u = 128 + u;
  if (u < 0) u = 0;
  if (u > 255) u = 255;
  return (int)floor(.5 + u);
}

/* common.h:37-45 */
float host_ulaw2lin(float u)
{
  float scale_1 = 32768.f / 255.f;
  u = u - 128.f;
  float s = u >= 0.f ? 1.f : -1.f;
  u = fabsf(u);
  return s * scale_1 * (exp(u / 128. * 5.5451774445f) - 1);
}

int check_constants(const ModelConst &mc)
{
  if (!std::isfinite(mc.lpc_gamma)) { set_err("LPC_GAMMA must be finite"); return -1; }
  if (mc.delay < 0 || mc.delay > MAX_FEATURES_DELAY) {
    set_err("FEATURES_DELAY must lie in [0, " + std::to_string(MAX_FEATURES_DELAY) + "]");
    return -1;
  }
  if (mc.end2end != 0 && mc.end2end != 1) { set_err("END2END must be 0 or 1"); return -1; }
  return 0;
}

bool parse_blob(std::vector<Arr> &out, const unsigned char *data, int len)
{
  while (len > 0) {
    if (len < 64) return false;
    int size, block;
    memcpy(&size, data + 12, 4);
    memcpy(&block, data + 16, 4);
    if (block < size || block > len - 64 || data[63] != 0 || size <= 0) return false;
    out.push_back(Arr{std::string((const char *)data + 20), size, data + 64});
    data += block + 64;
    len -= block + 64;
  }
  return true;
}

const Arr *find(const std::vector<Arr> &l, const char *name)
{
  for (const Arr &a : l)
    if (a.name == name) return &a;
  return nullptr;
}

const void *find_check(const std::vector<Arr> &l, const char *name, int size)
{
  const Arr *a = find(l, name);
  if (!a || a->size != size) {
    set_err(std::string("weight array missing or mis-sized: ") + name);
    return nullptr;
  }
  return a->data;
}

bool parse_idx(const std::vector<Arr> &l, const char *name, int nb_in, int nb_out, std::vector<std::vector<int>> &blocks)
{
  const Arr *a = find(l, name);
  if (!a) { set_err(std::string("missing ") + name); return false; }
  std::vector<int> idx(a->size / 4);
  memcpy(idx.data(), a->data, idx.size() * 4);
  size_t p = 0;
  int remain = (int)idx.size();
  blocks.clear();
  while (remain > 0) {
    int nb = idx[p++];
    if (nb < 0 || remain < nb + 1) { set_err(std::string("bad idx ") + name); return false; }
    std::vector<int> pos(nb);
    for (int k = 0; k < nb; k++) {
      pos[k] = idx[p++];
      if (pos[k] + 3 >= nb_in || (pos[k] & 3) || pos[k] < 0) { set_err(std::string("bad idx pos ") + name); return false; }
    }
    blocks.push_back(pos);
    nb_out -= 8;
    remain -= nb + 1;
  }
  if (nb_out != 0) { set_err(std::string("idx rows mismatch ") + name); return false; }
  return true;
}

int total_blocks(const std::vector<std::vector<int>> &b)
{
  int t = 0;
  for (auto &v : b) t += (int)v.size();
  return t;
}

bool block_may_saturate(const int8_t *w)
{
  for (int r = 0; r < 8; r++)
    for (int c = 0; c < 4; c += 2) {
      int a = w[r * 4 + c], bb = w[r * 4 + c + 1];
      int pos = std::max(a, 0) + std::max(bb, 0), neg = std::max(-a, 0) + std::max(-bb, 0);
      if (255 * pos > 32767 || 255 * neg > 32768) return true;
    }
  return false;
}

static std::vector<int> row_starts(const std::vector<std::vector<int>> &blocks)
{
  std::vector<int> first(blocks.size() + 1, 0);
  for (size_t r = 0; r < blocks.size(); r++) first[r + 1] = first[r] + (int)blocks[r].size();
  return first;
}

/* the weight record of A.blocks: variant, prefix sums */
static int gru_a_weights(const std::vector<Arr> &L, GruASparse &A)
{
  A.nb = total_blocks(A.blocks);
  const Arr *gaw = find(L, "sparse_gru_a_recurrent_weights");
  if (!gaw) { set_err("missing sparse_gru_a_recurrent_weights"); return -1; }
  if (gaw->size == 32 * A.nb) A.variant = LPCNET_VARIANT_INT8;
  else if (gaw->size == 32 * A.nb * 4) A.variant = LPCNET_VARIANT_FP32;
  else { set_err("sparse_gru_a_recurrent_weights size matches neither int8 nor fp32"); return -1; }
  A.w = gaw->data;
  A.first = row_starts(A.blocks);
  return 0;
}

int parse_gru_a(const std::vector<Arr> &L, GruASparse &A)
{
  if (!parse_idx(L, "sparse_gru_a_recurrent_weights_idx", NA, GA_ROWS, A.blocks)) return -1;
  return gru_a_weights(L, A);
}

namespace {

/* The load path's hooks, read once per build. */
struct LoadEnv {
  bool no_quad = getenv("LPCNET_NO_QUAD") != nullptr;   /* A/B switch: per-slot LDS layout */
  bool no_mfma = getenv("LPCNET_NO_MFMA") != nullptr;
  bool no_fpk = getenv("LPCNET_NO_FPK") != nullptr;
  bool fp_force_long = getenv("LPCNET_FP_FORCE_LONG") != nullptr; /* tests: the long form on any model */
  bool fc_exact = false;                                           /* test hook: force the exact form */
  /* test hooks: force the exact path everywhere, or lower the z/r bound so
   * that some workgroups take each path */
  bool mf_exact = getenv("LPCNET_MF_EXACT") != nullptr;
  const char *mf_zr_bound = getenv("LPCNET_MF_ZR_BOUND");
  bool no_mfw_split = getenv("LPCNET_NO_MFW_SPLIT") != nullptr;
  bool rcp_host = false; /* LPCNET_RCP=host: this host's rcpps at load time */
  /* LPCNET_LPC_GAMMA / LPCNET_FEATURES_DELAY / LPCNET_END2END override the
   * blob's records and the defaults (drop-in callers) */
  const char *lpc_gamma = getenv("LPCNET_LPC_GAMMA"), *delay = getenv("LPCNET_FEATURES_DELAY"), *end2end = getenv("LPCNET_END2END");
  bool verbose = getenv("LPCNET_VERBOSE") != nullptr;
  MfPlanParams plan = mf_plan_params_from_env();
  LoadEnv()
  {
    const char *fe = getenv("LPCNET_FC_EXACT");
    fc_exact = fe && atoi(fe);
    const char *e = getenv("LPCNET_RCP");
    rcp_host = e && !strcmp(e, "host");
  }
};

/* The blob's records as the build reads them. */
struct Blob {
  GruASparse ga;
  std::vector<std::vector<int>> gb_blocks;
  std::vector<int> gb_first;
  int nbb = 0;
  bool int8 = false;
  const float *conv1_w, *conv2_w, *dense1_w, *dense2_w;
  const float *ga_bias, *ga_subias, *ga_diag, *gb_bias, *gb_subias, *fc_b, *fc_w, *fc_f;
  const void *gbw;
};

/* model constants: optional side records named like the #defines
 * dump_lpcnet.py:423-446 writes into nnet_data.h (LPC_GAMMA float,
 * FEATURES_DELAY int, END2END int; the reference's parser ignores unknown
 * records), else the dump defaults; the environment overrides both.  -1 on a
 * malformed record or an unsupported value. */
int model_constants(const std::vector<Arr> &L, const LoadEnv &env, ModelConst &mc)
{
  if (const Arr *a = find(L, "LPC_GAMMA")) {
    if (a->size != 4) { set_err("LPC_GAMMA record must hold one float"); return -1; }
    memcpy(&mc.lpc_gamma, a->data, 4);
  }
  if (const Arr *a = find(L, "FEATURES_DELAY")) {
    if (a->size != 4) { set_err("FEATURES_DELAY record must hold one int"); return -1; }
    memcpy(&mc.delay, a->data, 4);
  }
  if (const Arr *a = find(L, "END2END")) {
    if (a->size != 4) { set_err("END2END record must hold one int"); return -1; }
    memcpy(&mc.end2end, a->data, 4);
  }
  if (env.lpc_gamma) mc.lpc_gamma = strtof(env.lpc_gamma, nullptr);
  if (env.delay) mc.delay = atoi(env.delay);
  if (env.end2end) mc.end2end = atoi(env.end2end);
  return check_constants(mc);
}

/* records, sizes, variant, constants, codebooks */
int parse_model(const unsigned char *data, int len, const ModelBuildOpts &opts, const LoadEnv &env, Blob &B, HostModel &H)
{
  std::vector<Arr> &L = H.records;
  L.clear();
  if (!data || len <= 0 || !parse_blob(L, data, len)) {
    set_err("malformed weight blob");
    return -1;
  }
  /* the GRU_B index is checked before the GRU_A weight record, as ever */
  if (!parse_idx(L, "sparse_gru_a_recurrent_weights_idx", NA, GA_ROWS, B.ga.blocks)) return -1;
  if (!parse_idx(L, "gru_b_weights_idx", NA, GB_ROWS, B.gb_blocks)) return -1;
  if (gru_a_weights(L, B.ga)) return -1;
  B.nbb = total_blocks(B.gb_blocks);
  B.gb_first = row_starts(B.gb_blocks);
  H.variant = B.ga.variant;
  H.nba = B.ga.nb;
  H.nbb = B.nbb;
  B.int8 = H.variant == LPCNET_VARIANT_INT8;
  const int q = B.int8 ? 1 : 4;
#define F(var, name, cnt) if (!(var = (const float *)find_check(L, name, (cnt)*4))) return -1
  const float *embed_sig;
  F(B.conv1_w, "feature_conv1_weights", 3 * FIN * COND);
  F(H.conv1_b, "feature_conv1_bias", COND);
  F(B.conv2_w, "feature_conv2_weights", 3 * COND * COND);
  F(H.conv2_b, "feature_conv2_bias", COND);
  F(B.dense1_w, "feature_dense1_weights", COND * COND);
  F(H.dense1_b, "feature_dense1_bias", COND);
  F(B.dense2_w, "feature_dense2_weights", COND * COND);
  F(H.dense2_b, "feature_dense2_bias", COND);
  F(H.gadf_w, "gru_a_dense_feature_weights", COND * GA_ROWS);
  F(H.gadf_b, "gru_a_dense_feature_bias", GA_ROWS);
  F(H.gbdf_w, "gru_b_dense_feature_weights", COND * GB_ROWS);
  F(H.gbdf_b, "gru_b_dense_feature_bias", GB_ROWS);
  F(H.embed_pitch, "embed_pitch_weights", 256 * EP);
  F(embed_sig, "embed_sig_weights", 256 * 128);
  F(H.emb_sig, "gru_a_embed_sig_weights", 256 * GA_ROWS);
  F(H.emb_pred, "gru_a_embed_pred_weights", 256 * GA_ROWS);
  F(H.emb_exc, "gru_a_embed_exc_weights", 256 * GA_ROWS);
  F(B.ga_bias, "sparse_gru_a_bias", 6 * NA);
  F(B.ga_subias, "sparse_gru_a_subias", 6 * NA);
  F(B.ga_diag, "sparse_gru_a_recurrent_weights_diag", 3 * NA);
  F(B.gb_bias, "gru_b_bias", 6 * NB);
  F(B.gb_subias, "gru_b_subias", 6 * NB);
  F(B.fc_b, "dual_fc_bias", 512);
  F(B.fc_w, "dual_fc_weights", 256 * 32);
  F(B.fc_f, "dual_fc_factor", 512);
#undef F
  (void)embed_sig;
  H.mc = ModelConst{1.0f, DEFAULT_FEATURES_DELAY, 0};
  if (opts.replan) H.mc = opts.mc;
  else if (model_constants(L, env, H.mc)) return -1;
  /* the 1.6 kb/s decoder's codebooks (lpcnet_private.h:109-112, generated
   * ceps_codebooks.c in the reference; lpcnet_enc.c:109-119, 709 give their
   * sizes): optional records -- a blob without them (or with mis-sized ones,
   * which the reference's parser would never bind either) still synthesises,
   * only lpcnet_decode refuses it */
  static const char *const cbn[4] = {"ceps_codebook1", "ceps_codebook2", "ceps_codebook3", "ceps_codebook_diff4"};
  H.cb_ok = true;
  for (int k = 0; k < 4; k++) {
    H.cb[k] = find(L, cbn[k]);
    H.cb_ok &= H.cb[k] && H.cb[k]->size == (k < 3 ? 1024 * (NBANDS - 1) : 4096 * NBANDS) * 4;
  }
  B.gbw = find_check(L, "gru_b_weights", 32 * B.nbb * q);
  H.gbrec = find_check(L, "gru_b_recurrent_weights", 3 * NB * NB * q);
  if (!B.gbw || !H.gbrec) return -1;
  return 0;
}

/* saturation, biases / diagonals, the int8 row sums */
void build_gru_params(const Blob &B, HostModel &H)
{
  const bool int8 = B.int8;
  const int nba = H.nba, nbb = H.nbb;
  const int8_t *wa = (const int8_t *)B.ga.w, *wb = (const int8_t *)B.gbw, *wr = (const int8_t *)H.gbrec;
  const std::vector<int> &ga_first = B.ga.first, &gb_first = B.gb_first;
  bool sat = false;
  if (int8) {
    for (int k = 0; k < nba && !sat; k++) sat |= block_may_saturate(wa + 32 * k);
    for (int k = 0; k < nbb && !sat; k++) sat |= block_may_saturate(wb + 32 * k);
    for (int k = 0; k < 3 * NB * NB / 32 && !sat; k++) sat |= block_may_saturate(wr + 32 * k);
  }
  H.sat = sat;
  const float *abias = int8 ? B.ga_subias : B.ga_bias; /* USE_SU_BIAS only with DOT_PROD */
  const float *bbias = int8 ? B.gb_subias : B.gb_bias;
  H.ga_par.assign(6 * NA, 0.f);
  H.gb_par.assign(2 * GB_ROWS, 0.f);
  H.ga_wsum.assign(3 * NA, 0);
  H.gb_wsum.assign(2 * GB_ROWS, 0);
  for (int g = 0; g < 3; g++)
    for (int i = 0; i < NA; i++) {
      H.ga_par[g * NA + i] = abias[3 * NA + g * NA + i];
      H.ga_par[(3 + g) * NA + i] = B.ga_diag[g * NA + i];
    }
  for (int r = 0; r < GB_ROWS; r++) {
    H.gb_par[r] = bbias[r];
    H.gb_par[GB_ROWS + r] = bbias[GB_ROWS + r];
  }
  if (int8 && !sat) {
    for (int rb = 0; rb < GA_ROWS / 8; rb++)
      for (int k = ga_first[rb]; k < ga_first[rb + 1]; k++)
        for (int r = 0; r < 8; r++)
          for (int c = 0; c < 4; c++) H.ga_wsum[rb * 8 + r] += 128 * wa[32 * k + r * 4 + c];
    for (int rb = 0; rb < GB_ROWS / 8; rb++)
      for (int k = gb_first[rb]; k < gb_first[rb + 1]; k++)
        for (int r = 0; r < 8; r++)
          for (int c = 0; c < 4; c++) H.gb_wsum[rb * 8 + r] += 128 * wb[32 * k + r * 4 + c];
    for (int rb = 0; rb < GB_ROWS / 8; rb++)
      for (int cb = 0; cb < NB / 4; cb++)
        for (int r = 0; r < 8; r++)
          for (int c = 0; c < 4; c++) H.gb_wsum[GB_ROWS + rb * 8 + r] += 128 * wr[32 * (rb * (NB / 4) + cb) + r * 4 + c];
  }
}

/* device form: t + (127 << 23), see rcp_x86_fix; the default is the Intel
 * table (11 bits, each entry twice); a custom table stays across reloads,
 * LPCNET_RCP=host selects this host's at load time */
int build_rcp(const ModelBuildOpts &opts, const LoadEnv &env, HostModel &H)
{
  if ((opts.rcp_custom || opts.replan) && opts.rcp_dev) {
    H.rcp_dev.assign(opts.rcp_dev, opts.rcp_dev + RCP_ENTRIES);
  } else {
    H.rcp_dev = default_rcp_dev();
    if (env.rcp_host) {
      std::vector<uint32_t> h(RCP_ENTRIES);
      if (lpcnet_mi355x_host_rcp_table(h.data(), RCP_ENTRIES) != 0) {
        set_err("LPCNET_RCP=host: this host's rcpps is not a 12-bit exponent-invariant table");
        return -1;
      }
      for (int i = 0; i < RCP_ENTRIES; i++) H.rcp_dev[i] = h[i] + kRcpBias;
    }
  }
  H.rcp_custom = H.rcp_dev != default_rcp_dev();
  return 0;
}

/* the LDS image under construction: sections appended 16-byte aligned */
struct Image {
  std::vector<unsigned char> &img;
  void align16() { img.resize((img.size() + 15) / 16 * 16, 0); }
  size_t put(const void *p, size_t n)
  {
    align16();
    size_t off = img.size();
    img.resize(off + n);
    if (n) memcpy(img.data() + off, p, n); /* an empty section (a wave without blocks in a gate) has no source */
    return off;
  }
};

/* blocks per lane for each (wave, gate) of the lockstep GRU_A layout */
void lockstep_row_lengths(const Blob &B, int gaK[SAMPLE_WAVES][3])
{
  for (int w = 0; w < SAMPLE_WAVES; w++)
    for (int g = 0; g < 3; g++) {
      int K = 0;
      for (int j = 0; j < 8; j++) K = std::max(K, (int)B.ga.blocks[g * (NA / 8) + w * 8 + j].size());
      gaK[w][g] = K;
    }
}

/* quad layout: wave w, gate g, group gi of 4 slots, lane l = 8*(row block in wave) + row.
 * The z, r and h groups of one wave are contiguous (weights and column
 * words alike), so the kernel runs them as one software-pipelined stream. */
void build_quad_layout(const Blob &B, const int gaK[SAMPLE_WAVES][3], Image &I, LockstepTables &lt)
{
  const std::vector<std::vector<int>> &ga_blocks = B.ga.blocks, &gb_blocks = B.gb_blocks;
  for (int w = 0; w < SAMPLE_WAVES; w++) {
    int K4[3], G = 0;
    for (int g = 0; g < 3; g++) {
      K4[g] = (gaK[w][g] + 3) / 4;
      lt.ga_K4[w][g] = K4[g];
      G += K4[g];
    }
    std::vector<uint32_t> q((size_t)std::max(G, 1) * 64 * 4, 0), c((size_t)std::max(G, 1) * 8, 0);
    int g0 = 0;
    for (int g = 0; g < 3; g++) {
      for (int l = 0; l < 64; l++) {
        const int j = l >> 3, r = l & 7, rb = g * (NA / 8) + w * 8 + j;
        for (int k = 0; k < (int)ga_blocks[rb].size(); k++) {
          memcpy(&q[((size_t)(g0 + k / 4) * 64 + l) * 4 + (k & 3)], (const int8_t *)B.ga.w + 32 * (B.ga.first[rb] + k) + 4 * r, 4);
          if (r == 0) c[(g0 + k / 4) * 8 + j] |= (uint32_t)(ga_blocks[rb][k] / 4) << (8 * (k & 3));
        }
      }
      g0 += K4[g];
    }
    const int qbase = (int)(I.put(q.data(), q.size() * 4) / 16);
    const int cbase = (int)(I.put(c.data(), c.size() * 4) / 4);
    for (int g = 0, acc = 0; g < 3; acc += K4[g], g++) {
      lt.ga_qoff[w][g] = qbase + acc * 64;
      lt.ga_coff[w][g] = cbase + acc * 8;
    }
  }
  for (int rb = 0; rb < GB_ROWS / 8; rb++) {
    std::vector<uint32_t> q((size_t)(REG_GB / 4) * 64 * 4, 0), c((size_t)(REG_GB / 4) * 8, 0);
    for (int l = 0; l < 64; l++) {
      const int r = l & 7, ks = l >> 3;
      for (int j = 0; j < REG_GB; j++) {
        const int k = ks + 8 * j;
        if (k >= (int)gb_blocks[rb].size()) continue;
        memcpy(&q[((size_t)(j / 4) * 64 + l) * 4 + (j & 3)], (const int8_t *)B.gbw + 32 * (B.gb_first[rb] + k) + 4 * r, 4);
        if (r == 0) c[(j / 4) * 8 + ks] |= (uint32_t)(gb_blocks[rb][k] / 4) << (8 * (j & 3));
      }
    }
    lt.gb_qoff[rb] = (int)(I.put(q.data(), q.size() * 4) / 16);
    lt.gb_coff[rb] = (int)(I.put(c.data(), c.size() * 4) / 4);
  }
}

/* The dual-FC walk's form for the matrix-core kernel (MfTables::fc_fin). */
void build_fc_bound(const Blob &B, const LoadEnv &env, HostModel &H)
{
  MfTables &mt = H.sample.mf;
  /* dual-FC node sums (nnet.c:193-199) are bounded by |bias| + 2 sum|w|
   * for GRU_B states within [-2, 2]: while that is finite and below
   * kTanhFinBound (2^30; every partial sum of the kernel's float chain is
   * bounded by it too), tanh8's flush and NaN selects are dead
   * (tanh_x86_fin_n).  Node 0 is never walked (nnet.c:190: i = (1 << b) | val)
   * but is bounded like the rest. */
  bool fin = true;
  double worst = 0;
  for (int c = 0; c < 2; c++)
    for (int i = 0; i < 256; i++) {
      double bd = fabs((double)B.fc_b[c * 256 + i]);
      for (int j = 0; j < 16; j++) bd += 2.0 * fabs((double)B.fc_w[i * 32 + c * 16 + j]);
      fin = fin && std::isfinite(bd) && bd < (double)kTanhFinBound;
      worst = std::isfinite(bd) ? std::max(worst, bd) : INFINITY;
    }
  mt.fc_fin = fin && !env.fc_exact ? 1 : 0;
  if (env.verbose) {
    char line[160];
    snprintf(line, sizeof line, "lpcnet: dual-FC walk: %s form (largest node bound %g, limit %g%s)\n",
             mt.fc_fin ? "select-free" : "exact", worst, (double)kTanhFinBound, env.fc_exact ? ", exact forced" : "");
    H.bounds_note += line;
  }
}

/* The lockstep kernel's LDS image: the fixed tables (rcpps, u-law, logit,
 * dual FC), then the GRU weights in the quad layout (reg) or per slot; fp32
 * GRU_A blocks go to ga_wf (global memory). */
void build_lockstep_image(const Blob &B, const LoadEnv &env, HostModel &H)
{
  const bool int8 = B.int8;
  const std::vector<std::vector<int>> &ga_blocks = B.ga.blocks, &gb_blocks = B.gb_blocks;
  LockstepTables &lt = H.sample.lockstep;
  std::vector<unsigned char> &img = H.img;
  img.assign(IMG_VAR, 0);
  memcpy(&img[IMG_RCP], H.rcp_dev.data(), RCP_ENTRIES * 4);
  for (int i = 0; i < 256; i++) {
    float u = host_ulaw2lin((float)i);
    memcpy(&img[IMG_ULAW + 4 * i], &u, 4);
    /* lpcnet.c:188-191 */
    float prob = .025f + .95f * i / 255.f;
    float lg = (float)-log((double)((1 - prob) / prob)); /* C double log, not logf */
    memcpy(&img[IMG_LOGIT + 4 * i], &lg, 4);
  }
  memcpy(&img[IMG_FCW], B.fc_w, 256 * 32 * 4);
  memcpy(&img[IMG_FCB], B.fc_b, 512 * 4);
  memcpy(&img[IMG_FCF], B.fc_f, 512 * 4);
  Image I{img};
  if (int8) lt.gb_rec_off = (int)I.put(H.gbrec, 3 * NB * NB);
  int gaK[SAMPLE_WAVES][3];
  lockstep_row_lengths(B, gaK);
  bool reg = int8;
  for (int w = 0; w < SAMPLE_WAVES; w++)
    for (int g = 0; g < 3; g++)
      if (gaK[w][g] > 96) reg = false;
  for (int rb = 0; rb < GB_ROWS / 8; rb++)
    if ((int)gb_blocks[rb].size() > 8 * REG_GB) reg = false;
  if (env.no_quad) reg = false;
  H.reg = reg;
  if (reg) build_quad_layout(B, gaK, I, lt);
  /* GRU_B input blocks: [rb][k][row] (u32 int8 row quads | float4 fp32 rows) */
  for (int rb = 0; rb < GB_ROWS / 8; rb++) {
    int nb = (int)gb_blocks[rb].size();
    lt.gb_nb[rb] = nb;
    if (reg) continue;
    if (int8) {
      std::vector<uint32_t> w(nb * 8);
      for (int k = 0; k < nb; k++)
        for (int r = 0; r < 8; r++) memcpy(&w[k * 8 + r], (const int8_t *)B.gbw + 32 * (B.gb_first[rb] + k) + 4 * r, 4);
      lt.gb_woff[rb] = (int)(I.put(w.data(), w.size() * 4) / 4);
    } else {
      std::vector<float> w(nb * 8 * 4);
      const float *src = (const float *)B.gbw;
      for (int k = 0; k < nb; k++)
        for (int r = 0; r < 8; r++)
          for (int c = 0; c < 4; c++) w[(k * 8 + r) * 4 + c] = src[32 * (B.gb_first[rb] + k) + c * 8 + r];
      lt.gb_woff[rb] = (int)(I.put(w.data(), w.size() * 4) / 4);
    }
    std::vector<uint16_t> cbs(nb);
    for (int k = 0; k < nb; k++) cbs[k] = (uint16_t)(gb_blocks[rb][k] / 4);
    lt.gb_coff[rb] = (int)(I.put(cbs.data(), cbs.size() * 2) / 2);
  }
  /* GRU_A blocks (LDS / fp32 global path): per (wave, gate) chunk [k][64 lanes] */
  std::vector<float4> &ga_wf = H.ga_wf;
  ga_wf.clear();
  for (int w = 0; w < SAMPLE_WAVES && !reg; w++)
    for (int g = 0; g < 3; g++) {
      int K = gaK[w][g];
      lt.ga_K[w][g] = K;
      std::vector<uint16_t> cbs(K * 8, int8 ? 0 : 0xFFFF);
      std::vector<uint32_t> wq(int8 ? K * 64 : 0, 0);
      size_t fbase = ga_wf.size();
      if (!int8) ga_wf.resize(fbase + (size_t)K * 64, make_float4(0, 0, 0, 0));
      for (int j = 0; j < 8; j++) {
        int rb = g * (NA / 8) + w * 8 + j;
        for (int k = 0; k < (int)ga_blocks[rb].size(); k++) {
          cbs[k * 8 + j] = (uint16_t)(ga_blocks[rb][k] / 4);
          for (int r = 0; r < 8; r++) {
            int blk = B.ga.first[rb] + k;
            if (int8) {
              memcpy(&wq[k * 64 + j * 8 + r], (const int8_t *)B.ga.w + 32 * blk + 4 * r, 4);
            } else {
              const float *src = (const float *)B.ga.w + 32 * blk;
              ga_wf[fbase + k * 64 + j * 8 + r] = make_float4(src[0 * 8 + r], src[1 * 8 + r], src[2 * 8 + r], src[3 * 8 + r]);
            }
          }
        }
      }
      if (int8) lt.ga_woff[w][g] = (int)(I.put(wq.data(), wq.size() * 4) / 4);
      else lt.ga_woff[w][g] = (int)fbase;
      lt.ga_coff[w][g] = (int)(I.put(cbs.data(), cbs.size() * 2) / 2);
    }
  I.align16();
  lt.image_bytes = (int)img.size();
}

void print_plan(bool mf_ok, const MfPlan &plan)
{
  fprintf(stderr, "lpcnet: mf_kernel plan: %s", !mf_ok ? "not applicable" : plan.split ? "split" : "unsplit");
  if (mf_ok) {
    fprintf(stderr, " own caps z/r %d h %d, pieces z %zu r %zu h %zu; groups per wave (own zr, hosted zr, own h, hosted h):",
            plan.own[0], plan.own[2], plan.pieces[0].size(), plan.pieces[1].size(), plan.pieces[2].size());
    for (int w = 0; w < SAMPLE_WAVES; w++) fprintf(stderr, " (%d %d %d %d)", plan.nzr[w], plan.nfzr[w], plan.nh[w], plan.nfh[w]);
    for (int g = 0; g < 3; g++) {
      std::vector<int> per(NA / 8, 0);
      for (const MfPiece &pc : plan.pieces[g]) per[pc.unit]++;
      fprintf(stderr, "%s max pieces per row %d", g ? "," : ";", per.empty() ? 0 : *std::max_element(per.begin(), per.end()));
    }
  }
  fprintf(stderr, "\n");
}

/* GRU_B of the matrix-core kernels: dense A tiles, lane l = row 16g + l%16,
 * k = 64kt + 16(l/16) + byte */
void build_mf_gru_b(const Blob &B, HostModel &H)
{
  const int8_t *wb = (const int8_t *)B.gbw, *wr = (const int8_t *)H.gbrec;
  std::vector<int8_t> dense((size_t)GB_ROWS * NA, 0), drec((size_t)GB_ROWS * NB, 0);
  for (int rb = 0; rb < GB_ROWS / 8; rb++)
    for (int t = 0; t < (int)B.gb_blocks[rb].size(); t++)
      for (int r = 0; r < 8; r++)
        for (int c = 0; c < 4; c++)
          dense[(size_t)(rb * 8 + r) * NA + B.gb_blocks[rb][t] + c] = wb[32 * (B.gb_first[rb] + t) + 4 * r + c];
  for (int rb = 0; rb < GB_ROWS / 8; rb++)
    for (int cb = 0; cb < NB / 4; cb++)
      for (int r = 0; r < 8; r++)
        for (int c = 0; c < 4; c++) drec[(rb * 8 + r) * NB + 4 * cb + c] = wr[32 * (rb * (NB / 4) + cb) + 4 * r + c];
  H.mf_gb.assign((size_t)MF_GB_TILES * 64 * 4, 0);
  for (int g = 0; g < 3; g++)
    for (int l = 0; l < 64; l++) {
      const int row = 16 * g + (l & 15), k0 = 16 * (l >> 4);
      for (int kt = 0; kt < 6; kt++)
        memcpy((int8_t *)&H.mf_gb[((size_t)(g * 6 + kt) * 64 + l) * 4], &dense[(size_t)row * NA + 64 * kt + k0], 16);
      if (k0 == 0) memcpy((int8_t *)&H.mf_gb[((size_t)(18 + g) * 64 + l) * 4], &drec[row * NB], 16);
    }
}

/* matrix-core tables (non-saturating int8 models: mf_kernel, mf2_kernel,
 * mfw_kernel) */
void build_matrix_core_tables(const Blob &B, const ModelBuildOpts &opts, const LoadEnv &env, HostModel &H)
{
  MfTables &mt = H.sample.mf;
  MfwTables &wt = H.sample.mfw;
  SampleForm &form = H.sample.form;
  bool mf_ok = B.int8 && !H.sat && !env.no_mfma;
  /* the matrix-core GRU_B is a dense tile: a row block listing one block
   * position twice (find_idx_check accepts it, and sparse_sgemv_accum8x4
   * adds both blocks) has no dense form -- the lockstep kernel runs such a
   * model, block by block as the reference does */
  for (int rb = 0; rb < GB_ROWS / 8 && mf_ok; rb++) {
    std::vector<int> pos = B.gb_blocks[rb];
    std::sort(pos.begin(), pos.end());
    if (std::adjacent_find(pos.begin(), pos.end()) != pos.end()) mf_ok = false;
  }
  MfPlan plan;
  if (mf_ok) {
    /* the plan's SIMD weights follow the kernel the batch will run (see
     * mf_plan): the wide kernel above one mf_kernel<4> round unless turned
     * off.  A split plan's own tables serve mf_kernel / mf2_kernel (class
     * cls); the wide kernel's split form gets tables of its own below */
    H.plan_wide = opts.wide;
    const int cls = opts.streams >= MF2_MIN_STREAMS ? 2 : opts.streams >= 1024 ? 1 : 0;
    mf_ok = mf_plan(B.ga.blocks, plan, env.plan, opts.wide ? 3 : cls, cls);
  }
  if (env.verbose) print_plan(mf_ok, plan);
  H.mf_ok = mf_ok;
  if (!mf_ok) return;
  const int8_t *wa = (const int8_t *)B.ga.w;
  mf_tables(B.ga.blocks, B.ga.first, wa, plan, H.mf);
  form.mf_split = plan.split ? 1 : 0;
  for (int g = 0; g < 3; g++) {
    H.mf_own[g] = plan.own[g];
    H.mf_pieces[g] = (int)plan.pieces[g].size();
  }
  for (int w = 0; w < SAMPLE_WAVES; w++) {
    mt.mf_nzr[w] = plan.nzr[w];
    mt.mf_nh[w] = plan.nh[w];
    mt.mf_nfzr[w] = plan.nfzr[w];
    mt.mf_nfh[w] = plan.nfh[w];
  }
  /* the wide kernel's split form (wide batches of split models) */
  form.mfw_split = 0;
  if (plan.split && H.plan_wide && !env.no_mfw_split && mfw_split_tables(B.ga.blocks, B.ga.first, wa, env.plan, H.mfw)) {
    form.mfw_split = 1;
    for (int w = 0; w < MFW_TAB_WAVES; w++) {
      wt.mfw_nzr[w] = H.mfw.nzr[w];
      wt.mfw_nh[w] = H.mfw.nh[w];
    }
  }
  build_mf_gru_b(B, H);
}

/* Range of the GRU_A gates' inputs for the elementwise fast path:
 * z/r: cvt_rne((bias + diag st + ((cond + Esig) + Epred) + Eexc) * 16256)
 * cannot leave int32 (x86: INT_MIN) while |that sum| < 2^31 / 16256, with
 * |st| <= 2 (restore-enforced); h: tanh's Pade denominator cannot overflow
 * nor go NaN while its input -- (bias + diag st + recurrent sum) r + (cond +
 * embeddings) -- is finite and below kTanhFinBound (2^30): the int8
 * recurrent sum is an int32 x 2^-14, below 2^17 in magnitude, and r lies in
 * [0, 1].  The kernel checks a workgroup's conditioning against these bounds
 * once per launch. */
void build_range_bounds(const LoadEnv &env, HostModel &H)
{
  MfTables &mt = H.sample.mf;
  double bz = 0, bh = 0, ez = 0, eh = 0;
  bool finite = true;
  for (int i = 0; i < NA; i++)
    for (int g = 0; g < 3; g++) {
      const double b = fabs((double)H.ga_par[g * NA + i]) + 2.0 * fabs((double)H.ga_par[(3 + g) * NA + i]);
      finite &= std::isfinite(b);
      (g < 2 ? bz : bh) = std::max(g < 2 ? bz : bh, b);
    }
  const float *tabs[3] = {H.emb_sig, H.emb_pred, H.emb_exc};
  for (int g = 0; g < 3; g++) {
    double e = 0;
    for (int t = 0; t < 3; t++) {
      double m = 0;
      for (int row = 0; row < 256; row++)
        for (int i = 0; i < NA; i++) {
          const float v = tabs[t][(size_t)row * GA_ROWS + g * NA + i];
          finite &= std::isfinite(v);
          m = std::max(m, (double)fabsf(v));
        }
      e += m;
    }
    (g < 2 ? ez : eh) = std::max(g < 2 ? ez : eh, e);
  }
  const double zr = 0.99 * (2147483648.0 / 16256.0) - bz - ez, hb = (double)kTanhFinBound - 0x1p17 - bh - eh;
  mt.mf_zr_bound = finite && zr > 0 ? (float)zr : -1.f;
  mt.mf_h_bound = finite && hb > 0 ? (float)hb : -1.f;
  if (env.mf_exact) mt.mf_zr_bound = mt.mf_h_bound = -1.f;
  if (env.mf_zr_bound) mt.mf_zr_bound = std::min(mt.mf_zr_bound, (float)atof(env.mf_zr_bound));
  if (env.verbose) {
    char line[200];
    snprintf(line, sizeof line, "lpcnet: GRU_A range bounds: z/r %g (bias+diag %g, embeddings %g), h %g\n", mt.mf_zr_bound, bz,
             ez, mt.mf_h_bound);
    H.bounds_note += line;
  }
}

/* an embedding table with its columns in lane order (coalesced gathers) */
std::vector<float> lane_ordered(const float *src, const std::vector<int> &units)
{
  std::vector<float> pt((size_t)256 * GA_ROWS);
  for (int row = 0; row < 256; row++)
    for (int g = 0; g < 3; g++)
      for (int p = 0; p < NA; p++) pt[(size_t)row * GA_ROWS + g * NA + p] = src[(size_t)row * GA_ROWS + g * NA + units[p]];
  return pt;
}

/* ---- fp32 latency-kernel tables (fp_kernel, see FP_ZF) ---- */

/* z / r weights of one slot as packed pairs: [z.x r.x z.y r.y] [z.z r.z z.w r.w] */
void fp_pack_zr(float4 &lo, float4 &hi, int g, const float4 &v)
{
  (g == 0 ? lo.x : lo.y) = v.x;
  (g == 0 ? lo.z : lo.w) = v.y;
  (g == 0 ? hi.x : hi.y) = v.z;
  (g == 0 ? hi.z : hi.w) = v.w;
}

/* Both forms: lane l of wave w = row l%8 of row block 8w + l/8 of each gate.
 * Sets the waves' slot counts and calls put(w, l, g, t, weights of the lane's
 * row in block t, column quad of block t) for every block of every lane. */
template <typename Put>
void fp_for_each_slot(const Blob &B, FpTables &ft, Put put)
{
  const std::vector<std::vector<int>> &ga_blocks = B.ga.blocks;
  const float *wa = (const float *)B.ga.w;
  for (int w = 0; w < SAMPLE_WAVES; w++) {
    int kz = 0, kh = 0;
    for (int j = 0; j < 8; j++) {
      kz = std::max(kz, (int)std::max(ga_blocks[w * 8 + j].size(), ga_blocks[NA / 8 + w * 8 + j].size()));
      kh = std::max(kh, (int)ga_blocks[2 * (NA / 8) + w * 8 + j].size());
    }
    ft.fp_nzr[w] = kz;
    ft.fp_nh[w] = kh;
    for (int l = 0; l < 64; l++) {
      const int j = l >> 3, r = l & 7;
      for (int g = 0; g < 3; g++) {
        const int rb = g * (NA / 8) + w * 8 + j;
        for (int t = 0; t < (int)ga_blocks[rb].size(); t++) {
          const float *src = wa + 32 * (size_t)(B.ga.first[rb] + t);
          put(w, l, g, t, make_float4(src[0 * 8 + r], src[1 * 8 + r], src[2 * 8 + r], src[3 * 8 + r]),
              (uint32_t)(ga_blocks[rb][t] / 4));
        }
      }
    }
  }
}

/* the register form: z/r slots in registers, h streamed, 4 offsets per word */
void build_fp_short(const Blob &B, HostModel &H)
{
  const float nz = -0.f;
  H.fp_zr.assign((size_t)SAMPLE_WAVES * 2 * FP_ZF * 64, make_float4(nz, nz, nz, nz));
  H.fp_h.assign((size_t)SAMPLE_WAVES * FP_HF * 64, make_float4(nz, nz, nz, nz));
  H.fp_off.assign((size_t)SAMPLE_WAVES * FP_OFF_WORDS * 64, 0x60606060u); /* column quad NA/4 = 96: the +0 quad */
  fp_for_each_slot(B, H.sample.fp, [&](int w, int l, int g, int t, const float4 &v, uint32_t q) {
    if (g < 2)
      fp_pack_zr(H.fp_zr[((size_t)w * 2 * FP_ZF + t) * 64 + l], H.fp_zr[((size_t)w * 2 * FP_ZF + FP_ZF + t) * 64 + l], g, v);
    else
      H.fp_h[((size_t)w * FP_HF + t) * 64 + l] = v;
    const int slot = g * FP_ZF + t, word = slot / 4, sh = 8 * (slot & 3);
    uint32_t &o = H.fp_off[((size_t)w * FP_OFF_WORDS + word) * 64 + l];
    o = (o & ~(0xFFu << sh)) | (q << sh);
  });
}

/* block rows longer than the register tables (trained masks, see mf_plan):
 * the long form streams every slot of the z/r and h chains.  [wave][slot][64
 * lanes]: z/r weights as the packed pairs (2 float4), h weights (float4);
 * offsets: z quad | r quad << 8, then h quad */
void build_fp_long(const Blob &B, HostModel &H)
{
  const std::vector<std::vector<int>> &ga_blocks = B.ga.blocks;
  const float nz = -0.f;
  int KZ = 1, KH = 1;
  for (int rb = 0; rb < NA / 8; rb++) {
    KZ = std::max(KZ, (int)std::max(ga_blocks[rb].size(), ga_blocks[NA / 8 + rb].size()));
    KH = std::max(KH, (int)ga_blocks[2 * (NA / 8) + rb].size());
  }
  H.fpl_zr.assign((size_t)SAMPLE_WAVES * KZ * 64 * 2, make_float4(nz, nz, nz, nz));
  H.fpl_h.assign((size_t)SAMPLE_WAVES * KH * 64, make_float4(nz, nz, nz, nz));
  H.fpl_off.assign((size_t)SAMPLE_WAVES * (KZ + KH) * 64, (uint32_t)(NA / 4) * 0x0101u); /* the +0 quad */
  fp_for_each_slot(B, H.sample.fp, [&](int w, int l, int g, int t, const float4 &v, uint32_t q) {
    if (g < 2) {
      fp_pack_zr(H.fpl_zr[(((size_t)w * KZ + t) * 64 + l) * 2], H.fpl_zr[(((size_t)w * KZ + t) * 64 + l) * 2 + 1], g, v);
      uint32_t &o = H.fpl_off[((size_t)w * KZ + t) * 64 + l];
      o = (o & ~(0xFFu << (8 * g))) | (q << (8 * g));
    } else {
      H.fpl_h[((size_t)w * KH + t) * 64 + l] = v;
      H.fpl_off[(size_t)SAMPLE_WAVES * KZ * 64 + ((size_t)w * KH + t) * 64 + l] = q;
    }
  });
  H.sample.fp.fpl_kz = KZ;
  H.sample.fp.fpl_kh = KH;
}

void build_fp_tables(const Blob &B, const LoadEnv &env, HostModel &H)
{
  const std::vector<std::vector<int>> &ga_blocks = B.ga.blocks, &gb_blocks = B.gb_blocks;
  bool fp_ok = !B.int8 && !env.no_fpk;
  for (int rb = 0; rb < GB_ROWS / 8 && fp_ok; rb++) {
    /* dense GRU_B only: blocks 0, 4, ..., NA-4 in order */
    if ((int)gb_blocks[rb].size() != NA / 4) fp_ok = false;
    for (int k = 0; k < (int)gb_blocks[rb].size() && fp_ok; k++)
      if (gb_blocks[rb][k] != 4 * k) fp_ok = false;
  }
  bool fp_long = false;
  for (int w = 0; w < SAMPLE_WAVES && fp_ok; w++)
    for (int j = 0; j < 8; j++) {
      if ((int)ga_blocks[w * 8 + j].size() > FP_ZF || (int)ga_blocks[NA / 8 + w * 8 + j].size() > FP_ZF ||
          (int)ga_blocks[2 * (NA / 8) + w * 8 + j].size() > FP_HF)
        fp_long = true;
    }
  if (env.fp_force_long) fp_long = true;
  H.fp_ok = fp_ok;
  H.fp_long = fp_long;
  H.sample.form.fp_long = fp_ok && fp_long ? 1 : 0;
  if (!fp_ok) return;
  if (fp_long) build_fp_long(B, H);
  else build_fp_short(B, H);
  /* dense GRU_B input weights, column quad major (both forms) */
  const float *wb = (const float *)B.gbw;
  H.fp_gb.resize((size_t)(NA / 4) * GB_ROWS);
  for (int rb = 0; rb < GB_ROWS / 8; rb++)
    for (int k = 0; k < NA / 4; k++)
      for (int r = 0; r < 8; r++) {
        const float *src = wb + 32 * (size_t)(B.gb_first[rb] + k);
        H.fp_gb[(size_t)k * GB_ROWS + rb * 8 + r] = make_float4(src[0 * 8 + r], src[1 * 8 + r], src[2 * 8 + r], src[3 * 8 + r]);
      }
}

/* choose streams per workgroup and check the LDS budget of the lockstep
 * kernel: the whole image in LDS, or -- models with long block rows -- only
 * its fixed tables, the weight sections read from global memory */
int choose_lockstep_lds(const ModelBuildOpts &opts, HostModel &H)
{
  auto lds_bytes = [&](int S, int image) { return image + opts.lds_extra[H.variant][S == 4 ? 2 : S == 2 ? 1 : 0]; };
  auto fit = [&](int image) {
    H.image_lds = image;
    H.S = opts.streams >= 1024 ? 4 : (opts.streams >= 512 ? 2 : 1);
    H.lds = lds_bytes(H.S, image);
    while (H.lds > 160 * 1024 && H.S > 1) {
      H.S /= 2;
      H.lds = lds_bytes(H.S, image);
    }
    return H.lds <= 160 * 1024;
  };
  if (!fit((int)H.img.size()) && !fit(IMG_VAR)) {
    set_err("model does not fit the 160 KiB LDS budget");
    return -1;
  }
  H.sample.lockstep.image_lds_bytes = H.image_lds;
  return 0;
}

/* frame-network weights keep the blob's [in][out] layout, padded with
 * FRAME_PREFETCH zero input rows: frame_kernel reads that far ahead */
std::vector<float> padded(const float *w, int nin, int nout)
{
  std::vector<float> v((size_t)(nin + FRAME_PREFETCH) * nout, 0.f);
  memcpy(v.data(), w, (size_t)nin * nout * 4);
  return v;
}

/* chunk_kernel's copies: each row tile's k steps as per-lane float4 quads
 * (one 1 KiB wave-instruction per 4 k steps instead of 256 B per step:
 * the kernel streams the weights from the Infinity Cache with 4x the
 * bytes in flight per CU) */
std::vector<float> tiled(const float *w, int nin, int nout)
{
  const int ks = nin / 4, nq = (ks + 3) / 4, nrt = nout / 16;
  std::vector<float> t((size_t)nrt * (nq + CK_WPAD) * 64 * 4, 0.f);
  for (int rt = 0; rt < nrt; rt++)
    for (int q = 0; q < nq; q++)
      for (int l = 0; l < 64; l++)
        for (int j = 0; j < 4; j++) {
          const int k = 4 * (4 * q + j) + (l >> 4), row = 16 * rt + (l & 15);
          if (k < nin) t[(((size_t)rt * (nq + CK_WPAD) + q) * 64 + l) * 4 + j] = w[(size_t)k * nout + row];
        }
  return t;
}

void build_frame_tables(const Blob &B, HostModel &H)
{
  H.conv1_p = padded(B.conv1_w, 3 * FIN, COND);
  H.conv2_p = padded(B.conv2_w, 3 * COND, COND);
  H.dense1_p = padded(B.dense1_w, COND, COND);
  H.dense2_p = padded(B.dense2_w, COND, COND);
  /* the two conditioning projections as one [COND][GA_ROWS + GB_ROWS] matrix */
  H.proj_w.assign((size_t)(COND + FRAME_PREFETCH) * (GA_ROWS + GB_ROWS), 0.f);
  H.proj_b.resize(GA_ROWS + GB_ROWS);
  for (int j = 0; j < COND; j++) {
    memcpy(&H.proj_w[(size_t)j * (GA_ROWS + GB_ROWS)], H.gadf_w + (size_t)j * GA_ROWS, GA_ROWS * 4);
    memcpy(&H.proj_w[(size_t)j * (GA_ROWS + GB_ROWS) + GA_ROWS], H.gbdf_w + (size_t)j * GB_ROWS, GB_ROWS * 4);
  }
  memcpy(H.proj_b.data(), H.gadf_b, GA_ROWS * 4);
  memcpy(H.proj_b.data() + GA_ROWS, H.gbdf_b, GB_ROWS * 4);
  /* conv1 .. dense2 once per projection slice of the one-frame kernel
   * (CK_SLICES_MAX copies): the slices of all 16-stream groups of an XCD
   * stream these rows in near lockstep, and one copy per slice spreads
   * their same-line L2 reads over four times the lines */
  auto rep = [](const std::vector<float> &t, int &quads) {
    std::vector<float> r;
    r.reserve(t.size() * CK_SLICES_MAX);
    for (int k = 0; k < CK_SLICES_MAX; k++) r.insert(r.end(), t.begin(), t.end());
    quads = (int)(t.size() / 4);
    return r;
  };
  H.ck_conv1 = rep(tiled(B.conv1_w, 3 * FIN, COND), H.ck_rep[0]);
  H.ck_conv2 = rep(tiled(B.conv2_w, 3 * COND, COND), H.ck_rep[1]);
  H.ck_dense1 = rep(tiled(B.dense1_w, COND, COND), H.ck_rep[2]);
  H.ck_dense2 = rep(tiled(B.dense2_w, COND, COND), H.ck_rep[3]);
  H.ck_proj = tiled(H.proj_w.data(), COND, GA_ROWS + GB_ROWS); /* the padding rows lie past its COND inputs */
}

/* algorithmic work, recomputed from the loaded index */
void build_info(const Blob &B, HostModel &H)
{
  const int nba = H.nba, nbb = H.nbb;
  const MfTables &mt = H.sample.mf;
  const SampleForm &form = H.sample.form;
  LPCNetModelInfo &in = H.info;
  in = LPCNetModelInfo{};
  in.variant = H.variant;
  in.gru_a_blocks = nba;
  in.gru_b_blocks = nbb;
  in.may_saturate = H.sat ? 1 : 0;
  in.quad_path = H.reg ? 1 : 0;
  double frame_w = (3.0 * FIN * COND + 3.0 * COND * COND + 2.0 * COND * COND + COND * GA_ROWS + COND * GB_ROWS) * 4 +
                   (2.0 * COND + 2 * COND + GA_ROWS + GB_ROWS) * 4 + EP * 4;
  double wbytes = B.int8 ? 1 : 4;
  in.bytes_shared_per_frame = frame_w;
  in.bytes_shared_per_sample = 32.0 * nba * wbytes + 4.0 * (nba + GA_ROWS / 8) /* idx */ + 6.0 * NA * 4 /* bias+diag */ +
                               32.0 * nbb * wbytes + 4.0 * (nbb + GB_ROWS / 8) + 3.0 * NB * NB * wbytes + 2.0 * GB_ROWS * 4;
  /* 3 gathered embedding rows, the 8 dual_fc nodes on the path (2
   * channels x (16 weights + bias + factor)), and the frame's conditioning +
   * features per sample, the output sample */
  in.bytes_per_stream_sample = 3.0 * GA_ROWS * 4 + 8 * 2 * (NB + 2) * 4 + (GA_ROWS + GB_ROWS + NF) * 4.0 / FRAME + 2;
  /* mf_kernel matrix-core work: per GRU_A wave 8 nzr + 4 nh 4x4x4 MFMAs of
   * 16 x 4x4x4 MACs; per sampler wave 21 16x16x64 MFMAs (2 sampler waves). */
  H.mf_ga_ops = H.mf_gb_ops = 0;
  if (H.mf_ok) {
    double n4 = 0;
    for (int w = 0; w < SAMPLE_WAVES; w++) n4 += 8.0 * (mt.mf_nzr[w] + mt.mf_nfzr[w]) + 4.0 * (mt.mf_nh[w] + mt.mf_nfh[w]);
    H.mf_ga_ops = 2.0 * n4 * 1024.0;
    H.mf_gb_ops = 2.0 * 2.0 * MF_GB_TILES * 16384.0;
  }
  in.long_rows = (H.mf_ok && form.mf_split) || (H.fp_ok && form.fp_long) ? 1 : 0;
  in.has_codebooks = H.cb_ok ? 1 : 0;
  in.lpc_gamma = H.mc.lpc_gamma;
  in.features_delay = H.mc.delay;
  in.end2end = H.mc.end2end;
  in.ops_per_sample = 2.0 * (32.0 * nba + 32.0 * nbb + 3 * NB * NB + 8 * 2 * NB + NLPC) +
                      2.0 * (3.0 * FIN * COND + 3.0 * COND * COND + 2.0 * COND * COND + COND * GA_ROWS + COND * GB_ROWS) / FRAME;
}

}  // namespace

int build_host_model(const unsigned char *data, int len, const ModelBuildOpts &opts, HostModel &H)
{
  const LoadEnv env;
  Blob B;
  H.sample = SampleTables{};
  if (parse_model(data, len, opts, env, B, H)) return -1;
  build_gru_params(B, H);
  if (build_rcp(opts, env, H)) return -1;
  build_fc_bound(B, env, H);
  build_lockstep_image(B, env, H);
  build_matrix_core_tables(B, opts, env, H);
  build_fp_tables(B, env, H);
  if (choose_lockstep_lds(opts, H)) return -1;
  build_frame_tables(B, H);
  if (H.mf_ok) {
    build_range_bounds(env, H);
    const float *src[3] = {H.emb_sig, H.emb_pred, H.emb_exc};
    for (int t = 0; t < 3; t++) {
      H.mf_emb[t] = lane_ordered(src[t], H.mf.units);
      if (H.sample.form.mfw_split) H.mfw_emb[t] = lane_ordered(src[t], H.mfw.units);
    }
  }
  if (H.cb_ok) {
    /* lpcnet_dec.c:118: float p = pow(2.f, main_pitch/21.)*PITCH_MIN_PERIOD, per 6-bit main_pitch */
    H.pitch.resize(64);
    for (int m = 0; m < 64; m++) H.pitch[m] = (float)(pow(2.0, m / 21.) * 32);
  }
  build_info(B, H);
  return 0;
}

std::vector<ModelUpload> model_uploads(const HostModel &h, ModelArgs &a)
{
  memset(&a.fa, 0, sizeof(a.fa));
  a.sample = h.sample;
  a.da = DecodeArgs{};
  for (int i = 0; i < 4; i++) a.fa.ck_rep[i] = h.ck_rep[i];
  std::vector<ModelUpload> up;
  auto raw = [&](void *dst, const void *src, size_t bytes, bool present) { up.push_back(ModelUpload{dst, src, bytes, present}); };
  auto vec = [&](void *dst, const auto &v, bool present = true) { raw(dst, v.data(), v.size() * sizeof(v[0]), present); };
  FrameArgs &fa = a.fa;
  SampleModel &sm = a.sample.model;
  LockstepTables &lt = a.sample.lockstep;
  MfTables &mt = a.sample.mf;
  MfwTables &wt = a.sample.mfw;
  FpTables &ft = a.sample.fp;
  const bool int8 = h.variant == LPCNET_VARIANT_INT8, mf = h.mf_ok, mfw = mf && h.sample.form.mfw_split;
  vec(&fa.conv1_w, h.conv1_p);
  raw(&fa.conv1_b, h.conv1_b, COND * 4, true);
  vec(&fa.conv2_w, h.conv2_p);
  raw(&fa.conv2_b, h.conv2_b, COND * 4, true);
  vec(&fa.dense1_w, h.dense1_p);
  raw(&fa.dense1_b, h.dense1_b, COND * 4, true);
  vec(&fa.dense2_w, h.dense2_p);
  raw(&fa.dense2_b, h.dense2_b, COND * 4, true);
  raw(&fa.gadf_w, h.gadf_w, COND * GA_ROWS * 4, true);
  raw(&fa.gadf_b, h.gadf_b, GA_ROWS * 4, true);
  raw(&fa.gbdf_w, h.gbdf_w, COND * GB_ROWS * 4, true);
  raw(&fa.gbdf_b, h.gbdf_b, GB_ROWS * 4, true);
  vec(&fa.proj_w, h.proj_w);
  vec(&fa.proj_b, h.proj_b);
  vec(&fa.ck_conv1, h.ck_conv1);
  vec(&fa.ck_conv2, h.ck_conv2);
  vec(&fa.ck_dense1, h.ck_dense1);
  vec(&fa.ck_dense2, h.ck_dense2);
  vec(&fa.ck_proj, h.ck_proj);
  raw(&fa.embed_pitch, h.embed_pitch, 256 * EP * 4, true);
  vec(&fa.rcp, h.rcp_dev);
  raw(&sm.emb_sig, h.emb_sig, 256 * GA_ROWS * 4, true);
  raw(&sm.emb_pred, h.emb_pred, 256 * GA_ROWS * 4, true);
  raw(&sm.emb_exc, h.emb_exc, 256 * GA_ROWS * 4, true);
  vec(&sm.ga_par, h.ga_par);
  vec(&sm.ga_wsum, h.ga_wsum);
  vec(&sm.gb_par, h.gb_par);
  vec(&sm.gb_wsum, h.gb_wsum);
  vec(&sm.image, h.img);
  vec(&mt.mf, h.mf.tab, mf);
  vec(&mt.mf_unit, h.mf.units, mf);
  vec(&mt.mf_frow, h.mf.frow, mf);
  vec(&wt.mfw_tab, h.mfw.tab, mfw);
  vec(&wt.mfw_frow, h.mfw.frow, mfw);
  vec(&wt.mfw_unit, h.mfw.units, mfw);
  for (int t = 0; t < 3; t++) vec(&mt.mf_emb[t], h.mf_emb[t], mf);
  for (int t = 0; t < 3; t++) vec(&wt.mfw_emb[t], h.mfw_emb[t], mfw);
  vec(&mt.mf_gb, h.mf_gb, mf);
  vec(&ft.fp_zr, h.fp_zr, h.fp_ok && !h.fp_long);
  vec(&ft.fp_h, h.fp_h, h.fp_ok && !h.fp_long);
  vec(&ft.fp_off, h.fp_off, h.fp_ok && !h.fp_long);
  vec(&ft.fpl_zr, h.fpl_zr, h.fp_ok && h.fp_long);
  vec(&ft.fpl_h, h.fpl_h, h.fp_ok && h.fp_long);
  vec(&ft.fpl_off, h.fpl_off, h.fp_ok && h.fp_long);
  vec(&ft.fp_gb, h.fp_gb, h.fp_ok);
  vec(&lt.ga_wf, h.ga_wf, !int8);
  raw(&sm.gb_recf, h.gbrec, 3 * NB * NB * 4, !int8);
  raw(&a.da.cb1, h.cb_ok ? h.cb[0]->data : nullptr, h.cb_ok ? h.cb[0]->size : 0, h.cb_ok);
  raw(&a.da.cb2, h.cb_ok ? h.cb[1]->data : nullptr, h.cb_ok ? h.cb[1]->size : 0, h.cb_ok);
  raw(&a.da.cb3, h.cb_ok ? h.cb[2]->data : nullptr, h.cb_ok ? h.cb[2]->size : 0, h.cb_ok);
  raw(&a.da.cbd, h.cb_ok ? h.cb[3]->data : nullptr, h.cb_ok ? h.cb[3]->size : 0, h.cb_ok);
  vec(&a.da.pitch, h.pitch, h.cb_ok);
  return up;
}

}  // namespace lpcnet_mi355x
