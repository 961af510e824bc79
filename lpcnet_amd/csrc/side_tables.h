/*
 * side_tables.h -- the host-built tables of what runs beside synthesis: the
 * constants of lpc_from_cepstrum (lpc_kernel.hip), of the feature extractor
 * (feat_kernel.hip) and of the Burg analysis (burg_kernel.hip), and the PLC
 * prediction network's records
 * re-tiled for plc_kernel.hip, and the DRED RDO-VAE's for rdovae_kernel.hip.
 * No device call: side_calls.cpp uploads them,
 * tools/model_host_check.cpp decodes the GRU tiles on the CPU.
 */
#ifndef LPCNET_SIDE_TABLES_H
#define LPCNET_SIDE_TABLES_H

#include <vector>

#include "model_host.h"
#include "side_kernels.h"

namespace lpcnet_mi355x {

/* both memset their table first: padding is defined */
void build_lpc_tables(LpcTables &T);
void build_feat_tables(FeatTables &T);
/* the encoder's main_pitch thresholds; a table of its own, in no digest */
void build_enc_tables(EncTables &T);
/* the Burg analysis' pow(.995, i + 1) doubles; a table of its own, in no digest */
void build_burg_tables(BurgTables &T);

/* One compute_gruB layer `nm` of nin inputs under the rules of gru_init and
 * find_idx_check: its units from the bias record, and with `tables` the A
 * tiles of its input (the idx expanded with zero blocks) and recurrent
 * weights and the seeds (side_kernels.h PlcArgs).  Units and inputs are
 * multiples of 64 up to PLC_DIM_MAX; int8 pairs that can saturate maddubs are
 * refused.  -1: set_err names the reason, prefixed with `who`. */
int gru_tiles_parse(const std::vector<Arr> &L, const std::string &who, const std::string &nm, int nin, bool tables, int &units,
                    std::vector<uint4> &g_in, std::vector<uint4> &g_rec, std::vector<int> &seed);

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

/* The DRED RDO-VAE's records (training_tf2/dump_rdovae.py with
 * keraslayerdump.py: <layer>_weights, _bias, and for GRUs _weights_idx,
 * _recurrent_weights, _subias), under the same rules.  Encoder (enc_dense1..8,
 * bits_dense, gdense1, gdense2) and decoder (state1..3, dec_dense1..8,
 * dec_final) are independent and optional; every dimension the generated
 * dred_rdovae_*_data.h would carry comes from the record sizes, and each
 * layer's input width must be its producer's output width.  A side that is
 * not usable has ok false and its reason in why. */
struct RdovaeGruHost {
  int in = 0, n = 0;
  std::vector<uint4> win, wrec;
  std::vector<int> seed;
};
struct RdovaeDenseHost {
  int in = 0, out = 0;
  const float *w = nullptr, *b = nullptr;
};
struct RdovaeSide {
  bool ok = false;
  std::string why;
  int in_dim = 0, T = 0, L = 0, S = 0, ksize = 0;
  int width[8] = {};
  RdovaeDenseHost d[5], head[4];
  RdovaeGruHost g[3];
};
struct RdovaeHost {
  RdovaeSide enc, dec;
};
/* 0 when at least one side is usable; -1 (set_err: both reasons) otherwise */
int rdovae_parse(const std::vector<Arr> &L, int variant, RdovaeHost &R, bool tables);
/* lpcnet_mi355x_rdovae_dims' array of a parsed model (zeros for a side that is not usable) */
constexpr int RDOVAE_DIMS = 24;
void rdovae_dims_of(const RdovaeHost &R, int dims[RDOVAE_DIMS]);
/* the device tables of one side: sets the scalars of `n` and returns one
 * entry per pointer member of it (dense w and b, GRU win, wrec and seed) */
std::vector<ModelUpload> rdovae_uploads(const RdovaeSide &S, RdovaeNet &n);

}  // namespace lpcnet_mi355x

#endif
