/*
 * model_host.h -- weight-blob ingest on the host: parsing and validation with
 * the reference's rules (parse_lpcnet_weights.c:36-113, 115-221) and every
 * table the kernels read, re-tiled from the blob into a HostModel.  No device
 * call: engine.cpp uploads a HostModel (model_uploads) and commits it to a
 * batch; tools/model_host_check.cpp checks one on the CPU.
 */
#ifndef LPCNET_MODEL_HOST_H
#define LPCNET_MODEL_HOST_H

#include <stdint.h>

#include <string>
#include <vector>

#include "device_mem.h"
#include "lpcnet_engine.h"
#include "lpcnet_mi355x.h"
#include "mf_plan.h"
#include "side_kernels.h" /* DecodeArgs */

namespace lpcnet_mi355x {

/* this thread's last error (lpcnet_mi355x_last_error) */
void set_err(const std::string &e);
const std::string &last_err();

/* the Intel build host's rcpps of the top 11 mantissa bits, and the device
 * table made of it (RCP_ENTRIES entries t + kRcpBias, each entry twice) */
extern const uint32_t kRcpTable[2048];
std::vector<uint32_t> default_rcp_dev();

/* host restatements of the scalar helpers used at init / reset */
int host_lin2ulaw(float x);
float host_ulaw2lin(float u);

/* ---- blob records (parse_lpcnet_weights.c:36-113) ---- */
struct Arr {
  std::string name;
  int size;
  const unsigned char *data;
};
bool parse_blob(std::vector<Arr> &out, const unsigned char *data, int len);
const Arr *find(const std::vector<Arr> &l, const char *name);
const void *find_check(const std::vector<Arr> &l, const char *name, int size);
/* find_idx_check: per 8-row block [nb, pos...], pos 4-aligned and < nb_in-3 */
bool parse_idx(const std::vector<Arr> &l, const char *name, int nb_in, int nb_out, std::vector<std::vector<int>> &blocks);
int total_blocks(const std::vector<std::vector<int>> &b);
/* pair sums of an int8 8x4 block that could saturate maddubs (x in [0,255]) */
bool block_may_saturate(const int8_t *w);
int check_constants(const ModelConst &mc);

/* The sparse GRU_A recurrent matrix of a blob: its block index, the prefix
 * sums of the block rows' lengths and the weight record; variant from the
 * record's size (int8: 32 bytes per block, fp32: 128).  -1 (set_err). */
struct GruASparse {
  std::vector<std::vector<int>> blocks; /* [3 NA / 8] block rows of input offsets */
  std::vector<int> first;               /* [rows + 1] */
  int nb = 0;
  int variant = 0;
  const unsigned char *w = nullptr;
};
int parse_gru_a(const std::vector<Arr> &L, GruASparse &A);

/* What a build takes from the batch and its device instead of reading them
 * where it needs them. */
struct ModelBuildOpts {
  int streams = 1;      /* the batch size: plan class and streams per workgroup */
  bool wide = false;    /* the batch will run mfw_kernel (kernel_choice.cpp plans_wide): plan class 3 and,
                           for split models, the wide split tables */
  /* replan: the batch's own blob again, for new register tables only: what
   * the caller set since the load -- the model constants, the rcpps table --
   * stays as it is, whatever the blob's records and the environment say */
  bool replan = false;
  ModelConst mc{1.0f, DEFAULT_FEATURES_DELAY, 0}; /* replan: the constants to keep */
  bool rcp_custom = false;                        /* the batch carries a custom rcpps table, which stays across reloads */
  const uint32_t *rcp_dev = nullptr;              /* rcp_custom or replan: that table (RCP_ENTRIES, device form) */
  /* sample_lds_bytes(S, variant, 0) for S = 1, 2, 4: the lockstep kernel's
   * LDS beside the image */
  int lds_extra[2][3] = {};
};

/* Everything a load computes.  The pointer members of `sample` are null; the
 * const pointers below look into the blob, which must outlive the model. */
struct HostModel {
  std::vector<Arr> records;
  int variant = 0;
  bool sat = false, reg = false, mf_ok = false, fp_ok = false, fp_long = false, cb_ok = false;
  bool plan_wide = false;
  ModelConst mc{1.0f, DEFAULT_FEATURES_DELAY, 0};
  int S = 1, lds = 0, image_lds = 0; /* lockstep kernel: streams per workgroup, LDS bytes, image bytes held in LDS */
  int nba = 0, nbb = 0;
  std::vector<uint32_t> rcp_dev;
  bool rcp_custom = false; /* rcp_dev is not the default table */
  SampleTables sample{}; /* the sample kernels' scalars, family by family, and the launchers' forms */
  int ck_rep[4] = {};
  LPCNetModelInfo info{}; /* the numbers that do not depend on the kernel choice */
  double mf_ga_ops = 0, mf_gb_ops = 0;
  std::string bounds_note; /* LPCNET_VERBOSE: the range-bounds line, printed when the model is uploaded */
  /* blob views */
  const float *conv1_b = nullptr, *conv2_b = nullptr, *dense1_b = nullptr, *dense2_b = nullptr;
  const float *gadf_w = nullptr, *gadf_b = nullptr, *gbdf_w = nullptr, *gbdf_b = nullptr;
  const float *embed_pitch = nullptr, *emb_sig = nullptr, *emb_pred = nullptr, *emb_exc = nullptr;
  const void *gbrec = nullptr;
  const Arr *cb[4] = {};
  /* frame network: padded [in + FRAME_PREFETCH][out], the projection gadf |
   * gbdf as one matrix, chunk_kernel's tiled (conv1 .. dense2 replicated) */
  std::vector<float> conv1_p, conv2_p, dense1_p, dense2_p, proj_w, proj_b;
  std::vector<float> ck_conv1, ck_conv2, ck_dense1, ck_dense2, ck_proj;
  /* sample kernels */
  std::vector<float> ga_par, gb_par;
  std::vector<int> ga_wsum, gb_wsum;
  std::vector<unsigned char> img;
  MfTab mf;
  int mf_own[3] = {}, mf_pieces[3] = {}; /* the plan behind mf: own caps in blocks and hosted pieces per gate (checks) */
  MfwSplitTab mfw;
  std::vector<uint32_t> mf_gb;
  std::vector<float> mf_emb[3], mfw_emb[3]; /* embedding tables in mf.units / mfw.units lane order */
  std::vector<float4> fp_zr, fp_h, fp_gb, fpl_zr, fpl_h, ga_wf;
  std::vector<uint32_t> fp_off, fpl_off;
  std::vector<float> pitch; /* the decoder's 64-entry pitch table */
};

/* Parse, validate and re-tile a weight blob.  0, or -1 (set_err) with `out`
 * in an unspecified state. */
int build_host_model(const unsigned char *data, int len, const ModelBuildOpts &opts, HostModel &out);

/* The device arguments of a model and the list of what to upload for them:
 * each entry is one device buffer, `bytes` of `src` whose address goes into
 * the pointer member at `dst`.  Entries that do not apply to the model
 * (present false) stay null.  The order is fixed (lpcnet_mi355x.h lists it
 * under lpcnet_mi355x_model_digest). */
struct ModelArgs {
  FrameArgs fa;
  SampleTables sample;
  DecodeArgs da;
};
/* struct ModelUpload: device_mem.h, beside DeviceTables::upload */
constexpr int MODEL_TABLES = 56;
/* sets the scalar members of `a` and returns the MODEL_TABLES entries */
std::vector<ModelUpload> model_uploads(const HostModel &h, ModelArgs &a);

/* FNV-1a-64 of a byte range */
uint64_t fnv1a64(const void *p, size_t n);

}  // namespace lpcnet_mi355x

#endif
