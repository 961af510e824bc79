/*
 * side_tables.h -- the host-built tables of what runs beside synthesis: the
 * constants of lpc_from_cepstrum (lpc_kernel.hip), of the feature extractor
 * (feat_kernel.hip) and of the Burg analysis (burg_kernel.hip), and the PLC
 * prediction network's records
 * re-tiled for plc_kernel.hip.  No device call: side_calls.cpp uploads them,
 * tools/model_host_check.cpp decodes the PLC tiles on the CPU.
 */
#ifndef LPCNET_SIDE_TABLES_H
#define LPCNET_SIDE_TABLES_H

#include <vector>

#include "model_host.h"

namespace lpcnet_mi355x {

/* both memset their table first: padding is defined */
void build_lpc_tables(LpcTables &T);
void build_feat_tables(FeatTables &T);
/* the encoder's main_pitch thresholds; a table of its own, in no digest */
void build_enc_tables(EncTables &T);
/* the Burg analysis' pow(.995, i + 1) doubles; a table of its own, in no digest */
void build_burg_tables(BurgTables &T);

/* The records of training_tf2/dump_plc.py:121-250 under the rules of
 * dense_init, gru_init and find_idx_check (parse_lpcnet_weights.c:90-171);
 * the dimensions the generated plc_data.h would carry come from the record
 * sizes.  Optional in a blob: -1 (set_err names the reason) means the PLC
 * calls refuse the model, never that synthesis does. */
struct PlcHost {
  int cond = 0, n[2] = {0, 0};
  const float *d1_w = nullptr, *d1_b = nullptr, *out_w = nullptr, *out_b = nullptr;
  std::vector<uint4> g_in[2], g_rec[2];
  std::vector<int> seed[2];
};
/* tables false: the checks and the dimensions only */
int plc_parse(const std::vector<Arr> &L, int variant, PlcHost &P, bool tables);

/* The device tables of a parsed predictor, in the style of model_uploads:
 * sets cond, n1 and n2 of `a` and returns the PLC_TABLES entries d1_w, d1_b,
 * g1_in, g1_rec, g1_seed, g2_in, g2_rec, g2_seed, out_w, out_b (all present). */
constexpr int PLC_TABLES = 10;
std::vector<ModelUpload> plc_uploads(const PlcHost &P, PlcArgs &a);

}  // namespace lpcnet_mi355x

#endif
