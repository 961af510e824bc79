/*
 * side_kernels.h -- the interfaces of the kernels beside synthesis: argument
 * structs, host-built tables and launchers of the LPC, packet decode, PLC
 * prediction, RDO-VAE, feature, Burg, encoder and concealment kernels.
 * Shared by their .hip files, the calls that launch them (synth_steps.cpp,
 * side_calls.cpp, conceal_calls.cpp) and the host code that builds their
 * tables (side_tables.cpp).
 */
#ifndef LPCNET_SIDE_KERNELS_H
#define LPCNET_SIDE_KERNELS_H

#include "lpcnet_engine.h" /* dimensions, StreamState */

namespace lpcnet_mi355x {

/* lpc_from_cepstrum on the device (lpc_kernel.hip).  Constant tables built
 * once per batch on the host (side_tables.cpp build_lpc_tables): the idct matrix
 * (freq.c dct_table), the 320-point kiss FFT twiddles and input permutation
 * (kiss_fft.c, lpcnet_tables.c), the band index and interpolation fraction of
 * every spectrum bin (freq.c:202-216), the compensation factors (freq.c:50). */
constexpr int LPC_NBANDS = NBANDS;
constexpr int LPC_WIN = 320;
constexpr int LPC_ORDER1 = NLPC + 1;
constexpr int LPC_CHUNK = 32;     /* frames per batched lpc_kernel launch (lpcnet_batch_synthesize_frames) */
/* FFT input slot i (after kiss_fft's digit reversal): spectrum bin
 * k = perm[i] (mirrored to 320 - k above 160), interpolated between band
 * energies `band` and band + 1 with fraction `frac` (band = NB_BANDS - 1 for
 * the zero bin 160), imaginary part -0.f for the mirrored (conjugate) bins. */
struct LpcSlot {
  float frac;
  unsigned char band, conj, pad[2];
};
struct LpcTables {
  double sqrt_2_18;               /* sqrt(2./NB_BANDS) (freq.c:238) */
  float scale;                    /* 1/320, kiss_fft's inverse scaling */
  float dct[LPC_NBANDS * LPC_NBANDS];
  float comp[LPC_NBANDS];
  float twr[LPC_WIN], twi[LPC_WIN];
  LpcSlot slot[LPC_WIN];
};
/* features [nstreams][NF] -> lpc_out [nstreams][NLPC] */
/* read-only matrices an idle-time kernel touches once per 128-byte line in
 * every XCD's L2 (the deferred lpc_kernel warms the one-frame chunk
 * kernel's weights for the next tick) */
struct L2Warm {
  const uint32_t *m[5];
  int lines[5];
};
int launch_lpc(const float *features, float *lpc_out, int nstreams, const LpcTables *tables, void *stream,
               StreamState *ring = nullptr, int ring_depth = 0, const L2Warm *warm = nullptr);

/* decode_packet (lpcnet_dec.c:81-156) on the device (decode_kernel.hip):
 * packets [npackets][nstreams][8] -> features [4 npackets][nstreams][NF],
 * each stream's vq_mem in st carried from packet to packet. */
struct DecodeArgs {
  const unsigned char *packets;
  int npackets, nstreams;
  StreamState *st;
  const float *cb1, *cb2, *cb3; /* ceps_codebook1..3 [1024][NBANDS - 1] */
  const float *cbd;             /* ceps_codebook_diff4 [4096][NBANDS] */
  const float *pitch;           /* [64]: (float)(pow(2.f, m / 21.) * PITCH_MIN_PERIOD) (lpcnet_dec.c:118) */
  float *features;
};
constexpr int DEC_MAX_PACKETS = LPC_CHUNK / 4; /* packets per decode launch (the frames of one chunk) */
int launch_decode(const DecodeArgs &a, void *stream);

/* The PLC prediction network (compute_plc_pred, lpcnet_plc.c:135-145) for a
 * whole batch (plc_kernel.hip): dense1 57 -> cond (tanh), two compute_gruB
 * layers cond -> n1 -> n2 (int8, DOT_PROD / USE_SU_BIAS numerics), plc_out
 * n2 -> NF (linear) and the out[19] boost.  One weight set for every stream;
 * a workgroup owns PLC_TILE streams, the N of v_mfma_i32_16x16x64_i8.
 * GRU weights as dense A tiles (the input idx expanded with zero blocks):
 * [unit tile ut][gate g][k tile kt][64 lanes] uint4, lane l = row g n + 16 ut
 * + l % 16, bytes k = 64 kt + 16 (l / 16) + 0..15 (mf_common.h mfma16).
 * seed [2][3 n] int32: rne(subias * SCALE) + 128 * rowsum(w) of the input
 * half, then of the recurrent half (x is consumed as u8 - 128). */
constexpr int PLC_IN = 2 * NBANDS + NF + 1; /* Burg cepstrum, features, loss flag */
constexpr int PLC_TILE = 16;                /* streams per workgroup */
constexpr int PLC_THREADS = 512;             /* 8 waves: 256 and 1024 measured slower at 8192+ streams (profiles/r08) */
constexpr int PLC_DIM_MAX = 512;            /* cond, n1, n2: multiples of 64 up to this */
struct PlcArgs {
  int nstreams;
  int cond, n1, n2;
  const float *in;             /* [B][PLC_IN]; null: all-zero input */
  float *out;                  /* [B][NF]; null: discarded */
  const unsigned char *active; /* [B]; null: every stream */
  float *state;                /* [B][n1 + n2]: plc_gru1_state, plc_gru2_state */
  const float *d1_w, *d1_b;    /* [PLC_IN][cond], [cond] */
  const uint4 *g1_in, *g1_rec;
  const int *g1_seed;
  const uint4 *g2_in, *g2_rec;
  const int *g2_seed;
  const float *out_w, *out_b;  /* [n2][NF], [NF] */
  const uint32_t *rcp;         /* RCP_ENTRIES-entry table in global memory (the table form) */
  int rcp_hw;                  /* as SampleForm::rcp_hw */
};
int plc_lds_bytes(int cond, int n1, int n2);
int launch_plc(const PlcArgs &a, void *stream);

/* The DRED RDO-VAE (dred_rdovae_enc.c:38-95, dred_rdovae_dec.c:37-98,
 * dred_rdovae.c:38-52) for a whole batch (rdovae_kernel.hip).  Encoder and
 * decoder share one stack of eight layers -- dense (tanh), GRU, dense, GRU,
 * dense, GRU, dense, dense -- whose outputs are concatenated into T floats;
 * the encoder's heads are the causal conv bits_dense (linear, latents) and
 * gdense1 -> gdense2 (tanh, the initial state), the decoder's the three state
 * layers (tanh, the GRU states from an initial state) and dec_final (linear,
 * four feature frames).  Dense weights are the blob's [in][out] floats, GRU
 * weights the PLC's A tiles and seeds (PlcArgs).  A workgroup owns PLC_TILE
 * streams. */
constexpr int RDOVAE_DIM_MAX = 512;  /* every layer width, L, S and gdense1 */
constexpr int RDOVAE_KSIZE_MAX = 8;  /* the conv's kernel size */
constexpr int RDOVAE_QFRAME = 4 * NF; /* dec_final's rows */
struct RdovaeDense {
  const float *w, *b; /* [in][out], [out] */
  int in, out;
};
struct RdovaeGru {
  const uint4 *win, *wrec;
  const int *seed;
  int in, n;
};
struct RdovaeNet {
  int in_dim;        /* 2 NF (encoder), L (decoder) */
  int T, nt;         /* the concatenation; the three GRUs' units together */
  int off[8];        /* each layer's offset in the concatenation */
  RdovaeDense d[5];  /* stack layers 1, 3, 5, 7, 8 */
  RdovaeGru g[3];    /* stack layers 2, 4, 6 */
  /* encoder: bits_dense (in = ksize T), gdense1, gdense2; decoder: state1..3, dec_final */
  RdovaeDense head[4];
  int ksize;         /* encoder: the conv's kernel size */
  int wmax;          /* the widest float row the kernel keeps in LDS */
};
struct RdovaeArgs {
  RdovaeNet net;
  int decoder;                 /* 0: one encoder call; 1: the decoder forms */
  int nstreams;
  const unsigned char *active; /* [B]; null: every stream */
  float *state;                /* [B][nt] GRU states: the streams' own, or decode_all's scratch */
  float *cat;                  /* [tiles][T][PLC_TILE] the concatenation, a scratch */
  /* encoder: the input is in[s * in_stream + f * in_frame + 0..NF) of frames f = 0, 1 */
  const float *in;
  size_t in_stream, in_frame;
  float *mem;                  /* [B][(ksize - 1) T] the conv's memory */
  float *latents, *init_state; /* [B][L], [B][S] */
  /* decoder: dec_init from d_init [B][S] when given, then nframes qframes:
   * latent f of stream s at d_lat[(s * nframes + f) * L], its qframe at
   * d_out[(s * nframes + f) * RDOVAE_QFRAME] */
  const float *d_init, *d_lat;
  float *d_out;
  int nframes;
  const uint32_t *rcp;
  int rcp_hw;
};
int rdovae_lds_bytes(const RdovaeNet &n);
int launch_rdovae(const RdovaeArgs &a, void *stream);

/* The single-frame feature extractor (preemphasis, compute_frame_features,
 * process_single_frame: lpcnet_enc.c:872-880, 488-577, 814-870, pcount = 0)
 * for a whole batch (feat_kernel.hip).  What of LPCNetEncState crosses frames
 * on that path, per stream, outside StreamState (the synthesis snapshots keep
 * their size); all zero after a reset (lpcnet_encoder_init). */
constexpr int NTF = 36;          /* NB_TOTAL_FEATURES */
constexpr int PITCH_MIN = 32;    /* PITCH_MIN_PERIOD (lpcnet_private.h:14) */
constexpr int PITCH_MAX = 256;   /* PITCH_MAX_PERIOD */
constexpr int PITCH_STATES = PITCH_MAX - PITCH_MIN; /* Viterbi states */
struct alignas(16) FeatState {
  float analysis_mem[FRAME];        /* the previous frame's preemphasised input */
  float exc[PITCH_MAX];             /* exc_buf[FRAME .. FRAME + PITCH_MAX) after the previous frame */
  float pitch_max_path[PITCH_MAX];  /* pitch_max_path[0] */
  float pitch_mem[NLPC];
  float mem_preemph, pitch_filt, pitch_max_path_all;
  int best_i;                       /* in [0, PITCH_STATES) */
};
/* host-built constants: half_window (dump_lpcnet_tables.c:83-84) and, per
 * spectrum bin below 160, (float)j/band_size (freq.c:141) */
struct FeatTables {
  float half_window[FRAME];
  float frac[FRAME];
  int band_start[NBANDS]; /* eband5ms[b] * WINDOW_SIZE_5MS (freq.c:45-48, 138) */
  int pad[2];
};
struct FeatArgs {
  int nstreams;
  const short *pcm;            /* [B][FRAME], or */
  const float *pcm_f;          /* [B][FRAME] when pcm is null */
  float *features;             /* stream s writes features[s * stride .. + row) */
  int row;                     /* NF or NTF */
  int stride;                  /* floats between two streams' rows, >= row (row: a dense [B][row]) */
  const unsigned char *active; /* [B]; null: every stream */
  FeatState *state;            /* [B] */
  const LpcTables *lpc_tab;
  const FeatTables *tab;
  /* the superframe form only (launch_feat_super): frame k of 4; features is
   * then [B][NF] (row = NF) of that frame */
  int k;
  float *xc_out;               /* [B][8][PITCH_MAX]: rows 2 k, 2 k + 1 written */
  float *fw_out;               /* [B][8] */
  float *lpc_out;              /* [B][NLPC] of frame k */
};
int launch_feat(const FeatArgs &a, void *stream);
int launch_feat_super(const FeatArgs &a, void *stream);

/* burg_cepstral_analysis (freq.c:156-199, burg.c:98-245) for a whole batch
 * (burg_kernel.hip): 160 samples per stream -> 18 sums and 18 differences of
 * the two half-frames' Burg cepstra.  No state, no weights.  The table is a
 * struct of its own, uploaded on first use, in no digest. */
constexpr int BURG_N = 2 * NBANDS;          /* floats per stream */
constexpr int BURG_LEN = FRAME / 2 - 1;     /* burg_in samples of a half-frame (len - 1) */
constexpr int BURG_NC = NLPC + 2;           /* C0, lags 1..16, the energy of the first 16 samples */
struct BurgTables {
  double pw[NLPC]; /* pow(.995, i + 1) (freq.c:174), the host's */
};
constexpr int BURG_FILL_ZERO = 1; /* +0.f into out[BURG_N .. BURG_N + NF) */
constexpr int BURG_FILL_FLAG = 2; /* flag into out[PLC_IN - 1] */
struct BurgArgs {
  int nstreams;
  const short *pcm;            /* [B][FRAME], or */
  const float *pcm_f;          /* [B][FRAME] when pcm is null */
  float *out;                  /* stream s writes out[s * stride .. + BURG_N) */
  int stride;                  /* >= BURG_N; >= PLC_IN with a fill */
  int fill;                    /* BURG_FILL_*: the rest of a predictor input row that starts at out */
  float flag;
  const unsigned char *active; /* [B]; null: every stream */
  const LpcTables *lpc_tab;
  const FeatTables *tab;
  const BurgTables *btab;
  /* scratch of one call, column 2 s + h of 2 B: the autocorrelations, the
   * recursion's 32 samples, then the filter input and the gain */
  double *cbuf;                /* [BURG_NC][2 B] */
  float *xbuf;                 /* [2 NLPC][2 B] */
  float *obuf;                 /* [NLPC + 1][2 B] */
};
int launch_burg(const BurgArgs &a, void *stream);
/* a predictor input row without its Burg part: +0.f into rows[s][0 .. BURG_N),
 * flag into rows[s][PLC_IN - 1] of every live stream; rows [B][PLC_IN] */
int launch_plc_row_fill(float *rows, float flag, const unsigned char *active, int nstreams, void *stream);

/* lpcnet_encode / lpcnet_compute_features after their four frame analyses:
 * process_superframe (lpcnet_enc.c:579-743) for a whole batch (enc_kernel.hip).
 * The scratch below is written and consumed within one packet of one call and
 * is no state; what crosses packets is FeatState (the Viterbi rows are the
 * single-frame path's) and each stream's encoder vq_mem.
 * Distances of 1e15f or more, and NaN, are outside the contract: the
 * reference then reads uninitialised indices (lpcnet_enc.c:53-78, 138-147);
 * here every index stays inside its codebook, and its value is unspecified.
 * PCM input cannot produce such distances. */
constexpr int ENC_PITCH_THR = 63; /* main_pitch = how many of these center_pitch reaches */
struct EncTables {
  float pitch_thr[ENC_PITCH_THR + 1]; /* ascending; [63] pads */
};
struct EncArgs {
  int nstreams;
  int quantize;                /* 1: lpcnet_encode (quantize = encode = 1); 0: lpcnet_compute_features */
  const unsigned char *active; /* [B]; null: every stream */
  FeatState *state;            /* [B] */
  float *vq_mem;               /* [B][NBANDS], the encoder's (not the decoder's) */
  float *xc;                   /* [B][8][PITCH_MAX] scratch: xc[2..9] */
  float *fw;                   /* [B][8] scratch: frame_weight[2..9] */
  float *feat;                 /* [4][B][NF] scratch: cepstra in, st->features[k][0..19] out */
  int *fields;                 /* [B][4] scratch: c0_id + 64, main_pitch, modulation field, corr_id */
  const float *lpc;            /* [4][B][NLPC] scratch (enc_out_kernel) */
  const EncTables *tab;
  const float *cb1, *cb2, *cb3, *cbd, *pitch; /* as DecodeArgs */
  unsigned char *packets;      /* [B][8]; null: not written */
  float *features;             /* [4][B][row]; null: not written */
  int row;                     /* NF or NTF */
};
/* the Viterbi pass over xc[2..9], backtrack, pitch regression and quantisation, c0 */
int launch_enc_pitch(const EncArgs &a, void *stream);
/* quantize_3stage_mbest, quantize_diff, double_interp_search,
 * perform_double_interp and bits_pack (quantize = 1 only) */
int launch_enc_vq(const EncArgs &a, void *stream);
/* live streams' rows of feat | lpc into features */
int launch_enc_out(const EncArgs &a, void *stream);
/* main_pitch of lpcnet_enc.c:678-679 from the threshold table, host and device alike */
__host__ __device__ inline int enc_main_pitch(const float *thr, float cp)
{
  int m = 0;
  if (cp < __builtin_inff()) /* inf: log = inf, floor, (int) = INT_MIN, IMIN, IMAX -> 0; NaN compares false */
    for (int i = 0; i < ENC_PITCH_THR; i++) m += cp >= thr[i];
  return m;
}

/* The data side of lpcnet_plc_update / lpcnet_plc_conceal between their
 * network and analysis calls (conceal_kernel.hip): per stream, beside
 * StreamState (the synthesis snapshots keep their size), what of
 * LPCNetPLCState (lpcnet_private.h:78-106) the three modes carry, and the
 * scratch a tick hands over through.  Every launcher takes the streams it
 * works on as an index list idx [n] in device memory; a stream appears in a
 * list at most once. */
constexpr int CONCEAL_FEC_ROWS = 100; /* PLC_MAX_FEC */
constexpr int CONCEAL_DEFER = 4;      /* MAX_FEATURE_BUFFER_SIZE */
struct ConcealData {
  int nstreams;
  int delay;          /* FEATURES_DELAY the buffers were laid out for */
  int buf;            /* PLC_BUF_SIZE = delay * FRAME + FRAME / 2 */
  int nt;             /* n1 + n2 floats of one PLCNetState */
  float *features;    /* [B][NF] st->features */
  short *pcm;         /* [B][buf + FRAME] st->pcm */
  double *dc;         /* [B][2] dc_mem, syn_dc */
  float *copy;        /* [B][delay + 1][nt] plc_copy */
  float *fec;         /* [B][CONCEAL_FEC_ROWS][NF] */
  float *defer;       /* [B][CONCEAL_DEFER][NF] the LPCNetState's feature_buffer */
  float *plc_state;   /* [B][nt] plc_net (the predictor's own state) */
  /* scratch of one tick */
  float *rows;        /* [B][PLC_IN] the predictor's input row */
  short *lp;          /* [B][FRAME] lpcnet_plc_update_causal's lp */
  int *delta;         /* [B] its delta; zero without the DC filter */
  short *tmp;         /* [B][FRAME / 2] the speculative half frame */
  const float *blend_w; /* [FRAME / 2] (float)(.5 - .5*cos(M_PI*i/80)), the host's cos */
  /* the non-causal mode (lpcnet_plc.c:339-492), null in the others: state */
  short *queued;      /* [B][FRAME] queued_samples */
  short *dc_buf;      /* [B][FRAME / 2] */
  /* and scratch of one tick */
  short *rev;         /* [B][FRAME] lpcnet_plc_update_non_causal's rev */
  double *mem_bak;    /* [B] its mem_bak */
  short *frame;       /* [B][FRAME] st->pcm[0 .. 160) as dense rows, for the analysis launch */
};
enum {
  CONCEAL_DC_REMOVE = 0,
  CONCEAL_DC_RESTORE = 1,
  CONCEAL_DC_CONCEAL = 2,
  /* the non-causal forms */
  CONCEAL_DC_REMOVE_BAK = 3,    /* :364-372: CONCEAL_DC_REMOVE that keeps mem_bak */
  CONCEAL_DC_REDO = 4,          /* :388-398 */
  CONCEAL_DC_CONCEAL_HALF = 5,  /* :480-488, syn_dc over pcm[80 .. 160) (:482) */
  CONCEAL_DC_CONCEAL_WHOLE = 6  /* :480-488, syn_dc over pcm[0 .. 160) (:484) */
};
/* the DC filter on io [B][FRAME] (lpcnet_plc.c:195-204, 283-287, 330-335; 363-372, 387-398, 479-489): one lane per stream */
int launch_conceal_dc(const ConcealData &d, const int *idx, int n, short *io, int mode, void *stream);
/* io[0 .. 80) += dc_buf, io[80 .. 160) += lp[0 .. 80), dc_buf = lp[80 .. 160) (:444-448) */
int launch_conceal_dc_restore_delayed(const ConcealData &d, const int *idx, int n, short *io, void *stream);
/* rev[i] = io[159 - i] (:403) */
int launch_conceal_reverse(const ConcealData &d, const int *idx, int n, const short *io, void *stream);
/* st->pcm[159 - i] = blend of itself and rev[i] + delta, i < 80 (:407-411) */
int launch_conceal_blend_back(const ConcealData &d, const int *idx, int n, void *stream);
/* queued_samples = st->pcm[80 .. 160), io[0 .. 80) (:417-418) */
int launch_conceal_queue_fill(const ConcealData &d, const int *idx, int n, const short *io, void *stream);
/* io[80 .. 160) = io[0 .. 80), io[0 .. 80) = st->pcm[80 .. 160), st->pcm[0 .. 160) = io as it was (:440-442) */
int launch_conceal_reorder(const ConcealData &d, const int *idx, int n, short *io, void *stream);
/* rows [B][FRAME] at dst_off = st->pcm[src_off .. + cnt): dst the io rows (:464) or d.frame */
int launch_conceal_export(const ConcealData &d, const int *idx, int n, short *dst, int dst_off, int src_off, int cnt, void *stream);
/* io[0 .. 80) = blend of io and tmp - delta (:225-229) */
int launch_conceal_blend(const ConcealData &d, const int *idx, int n, short *io, void *stream);
/* features[0] = MAX16(-10, features[0] + att_table[.]) (:318-319) */
int launch_conceal_attenuate(const ConcealData &d, const int *idx, int n, int loss_count, void *stream);
/* st->pcm[dst_off .. + cnt) = (src_buf ? st->pcm : io row)[src_off .. + cnt); the ranges may overlap */
int launch_conceal_move(const ConcealData &d, const int *idx, int n, const short *io, int dst_off, int src_buf, int src_off, int cnt,
                        void *stream);
/* plc_copy ring push (:305-306); plc_net = plc_copy[k] */
int launch_conceal_plc_push(const ConcealData &d, const int *idx, int n, void *stream);
int launch_conceal_plc_restore(const ConcealData &d, const int *idx, int n, int k, void *stream);
/* fec[pos] into features and into the row's columns 36..55, flag -1, zeros before (:149-157) */
int launch_conceal_fec_fetch(const ConcealData &d, const int *idx, int n, int pos, void *stream);
/* run_frame_network_deferred's buffer push: analysed ? rows[36 .. 56) : features, `fill` frames held before */
int launch_conceal_defer_push(const ConcealData &d, const int *idx, int n, int analysed, int fill, void *stream);
/* between the streams' rows and the work order [n][NF] / [n][N] a partial-batch
 * synthesis step runs on: w_feat (null: none) from feat[s * feat_stride ..),
 * w_pcm (null: none) from pcm[s * pcm_stride ..); the work order's w_pcm to
 * dst[s * dst_stride ..).  The callers bound the rows. */
int launch_conceal_gather_rows(const int *idx, int n, float *w_feat, const float *feat, int feat_stride, short *w_pcm, const short *pcm,
                               int pcm_stride, int N, void *stream);
int launch_conceal_scatter_rows(const int *idx, int n, const short *w_pcm, short *dst, int dst_stride, int N, void *stream);
/* lpcnet_reset_signal (lpcnet.c:226-233) on st[idx[k]]; ulaw0 = lin2ulaw(0.f) */
int launch_conceal_reset_signal(StreamState *st, const int *idx, int n, int ulaw0, void *stream);
/* lpcnet_plc_fec_add's RNN_MOVE (:121) and RNN_COPY (:126) on one stream */
int launch_conceal_fec_compact(const ConcealData &d, int s, int from, int rows, void *stream);
int launch_conceal_fec_store(const ConcealData &d, int s, int pos, const float *features /* host, [NF] */, void *stream);

}  // namespace lpcnet_mi355x

#endif
