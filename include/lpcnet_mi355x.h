/*
 * lpcnet_mi355x.h -- batch extension and tooling of liblpcnet_mi355x.so.
 *
 * The reference has no batch API (one LPCNetState = one stream on one core,
 * SURVEY.md section 8b).  A batch owns B independent streams, each with
 * exactly the semantics of one reference LPCNetState; stream s of a batch is
 * PCM-identical to the same stream run alone through lpcnet_synthesize().
 * Streams shard across GPUs with no collective (one batch per device).
 */
#ifndef LPCNET_MI355X_H
#define LPCNET_MI355X_H

#include "lpcnet.h"
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct LPCNetBatch LPCNetBatch;

/* Weight-blob variants (chosen from the array sizes of the blob). */
#define LPCNET_VARIANT_INT8 0 /* reference AVX2 build: DOT_PROD int8 GRU weights */
#define LPCNET_VARIANT_FP32 1 /* reference --disable-dot-product build */

typedef struct {
  int variant;          /* LPCNET_VARIANT_* */
  int gru_a_blocks;     /* 8x4 blocks in sparse_gru_a_recurrent_weights */
  int gru_b_blocks;     /* 8x4 blocks in gru_b_weights */
  int may_saturate;     /* 1 if an int8 pair can saturate the int16 maddubs sum */
  double bytes_shared_per_frame;  /* algorithmic weight bytes read once per frame step */
  double bytes_shared_per_sample; /* algorithmic weight bytes read once per sample step (SURVEY 8d;
                                     add bytes_shared_per_frame / 160 for the whole step) */
  double bytes_per_stream_sample; /* per-stream bytes per sample (3 embedding rows, dual_fc path,
                                     conditioning/features/PCM share; SURVEY 8d: 15,009) */
  double ops_per_sample;          /* 2*MAC per stream per sample */
  int streams_per_workgroup;      /* streams per sample-kernel workgroup */
  int quad_path;                  /* sample kernel: 0 lockstep (per-slot LDS layout), 1 lockstep (quad
                                     LDS layout), 4 mf_kernel (matrix cores), 5 fp_kernel (fp32),
                                     6 mf2_kernel (matrix cores, two staggered 4-stream groups per
                                     workgroup; batches >= 2048; launches with preload or trace
                                     take mf_kernel), 7 mfw_kernel (two or three 4-stream groups per
                                     workgroup, chosen by cost -- two in the common case -- with dedicated
                                     gather/elementwise, recurrent and sampler waves; batches above one
                                     mf_kernel<4> round (> 4 streams per CU, i.e. > 1024 streams),
                                     non-split models, default rcpps; the same launches as 6) */
  int lds_bytes;                  /* dynamic LDS of the sample kernel */
  double mfma_ops_per_group_sample; /* int8 matrix-core ops issued per workgroup per sample
                                       (mf_kernel; padding included), 0 otherwise */
  /* model constants (see lpcnet_batch_set_model_constants) */
  float lpc_gamma;
  int features_delay;
  int end2end;
  /* 1: block rows longer than the fast kernels' register tables (trained
   * Sparsify masks): mf_kernel runs its split form, fp_kernel its streamed
   * (long) form */
  int long_rows;
  /* 1: the blob carries the 1.6 kb/s decoder's codebooks (ceps_codebook1..3,
   * ceps_codebook_diff4), so lpcnet_decode / lpcnet_batch_decode* accept it */
  int has_codebooks;
  /* 1: the fast kernels may use the hardware reciprocal for rcpps (the
   * default Intel table); 0: a custom table is set and they run their
   * table-only forms (the `HWR` template argument rocprofv3 shows) */
  int rcp_hw;
} LPCNetModelInfo;

/* Create a batch of nb_streams streams on HIP device `device`.
 * Returns NULL if the device is unavailable or nb_streams < 1. */
LPCNET_EXPORT LPCNetBatch *lpcnet_batch_create(int nb_streams, int device);
LPCNET_EXPORT void lpcnet_batch_destroy(LPCNetBatch *b);
/* 0 on success, -1 on a missing / mis-sized array (lpcnet_load_model rules). */
LPCNET_EXPORT int lpcnet_batch_load_model(LPCNetBatch *b, const unsigned char *data, int len);
LPCNET_EXPORT int lpcnet_batch_model_info(const LPCNetBatch *b, LPCNetModelInfo *info);
/* Sample-kernel selection: 0 automatic (default; env LPCNET_KERNEL),
 * 1 the lockstep kernel (every model: the fallback for saturating int8 models
 * and fp32 models with a sparse GRU_B), 4 mf_kernel (both int8 products on
 * the matrix cores; non-saturating int8 models whose blocks fit its register
 * tables), 5 fp_kernel (fp32 models with a dense GRU_B whose blocks fit its
 * tables).  Automatic: 5 where it applies, else 4 where it applies, else 1;
 * a forced mode the model cannot run falls back to 1.  Results are
 * identical; only speed differs.  Returns -1 for any other mode. */
LPCNET_EXPORT int lpcnet_batch_set_kernel(LPCNetBatch *b, int mode);
/* The model constants the reference compiles in from the generated
 * nnet_data.h (training_tf2/dump_lpcnet.py:423-446): LPC_GAMMA
 * (lpc_weighting of the frame's LPC, lpcnet.c:116-118), FEATURES_DELAY (the
 * lookahead: depth of the lpc_from_cepstrum ring, conv2 clear and silent
 * first frames, lpcnet.c:101,109-114,239; 0..4) and END2END (LPC from the
 * frame network's rc outputs via rc2lpc, lpcnet.c:56-80,107-108).
 * lpcnet_batch_load_model / lpcnet_load_model take them from optional blob
 * records named LPC_GAMMA (one float), FEATURES_DELAY and END2END (one int
 * each) -- the reference's parser skips records it does not bind -- else
 * the dump defaults (1.0, 2, 0); the environment variables LPCNET_LPC_GAMMA,
 * LPCNET_FEATURES_DELAY and LPCNET_END2END override both at load time.  This
 * setter changes them for the loaded model (until the next load; the
 * register tables that lpcnet_batch_set_kernel / _set_rcp_table may re-plan
 * are no load: the constants stay).  Returns -1 without a model or for an
 * unsupported value. */
LPCNET_EXPORT int lpcnet_batch_set_model_constants(LPCNetBatch *b, float lpc_gamma, int features_delay, int end2end);
/* lpcnet_reset() on every stream / on one stream. */
LPCNET_EXPORT void lpcnet_batch_reset(LPCNetBatch *b);
LPCNET_EXPORT int lpcnet_batch_reset_stream(LPCNetBatch *b, int stream);
LPCNET_EXPORT int lpcnet_batch_nb_streams(const LPCNetBatch *b);

/* One frame for every stream, host buffers: features [B][NB_FEATURES],
 * pcm [B][N], N <= 160.  Equivalent to lpcnet_synthesize() on each stream.
 * Returns 0, or -1 on error (no model, bad N). */
LPCNET_EXPORT int lpcnet_batch_synthesize(LPCNetBatch *b, const float *features, short *pcm, int N);

/* The batch's own host-addressable buffers for a live server's tick
 * (features [B][NB_FEATURES], PCM [B][160]; allocated on first use, freed
 * with the batch, NULL on error).  lpcnet_batch_synthesize with these
 * pointers skips its host staging copies: the kernels read the features
 * where they are, and the sample kernel stores the PCM into the (mapped,
 * pinned) PCM buffer itself where its write-out is coalesced -- no
 * device-to-host copy.  The feature buffer is host-visible device memory on
 * a large-BAR device (write it from the host; reads back are slow uncached
 * PCIe reads; LPCNET_FEAT_VRAM=0: mapped pinned host memory instead).  The
 * PCM buffer holds a frame's output until the next synthesis call. */
LPCNET_EXPORT float *lpcnet_batch_host_features(LPCNetBatch *b);
LPCNET_EXPORT short *lpcnet_batch_host_pcm(LPCNetBatch *b);

/* lpcnet_synthesize_impl (src/lpcnet.c:273-277, the PLC entry point): as
 * above, but the first `preload` samples of every stream are teacher-forced
 * from pcm (input), exactly as lpcnet.c:256-259; pcm[s][preload..N) is output.
 * N == 0 runs only the frame network (run_frame_network_flush, lpcnet.c:134). */
LPCNET_EXPORT int lpcnet_batch_synthesize_impl(LPCNetBatch *b, const float *features, short *pcm, int N, int preload);

/* lpcnet_synthesize_tail_impl (src/lpcnet.c:235-271, declared at
 * lpcnet_private.h:131): N samples of every stream from the conditioning and
 * LPC already in its state (no frame network); the first `preload` samples
 * teacher-forced from pcm as above. */
LPCNET_EXPORT int lpcnet_batch_synthesize_tail_impl(LPCNetBatch *b, short *pcm, int N, int preload);

/* run_frame_network (src/lpcnet.c:82-120) of one frame per stream, no samples.
 * update_conditions = 1: into the state's conditioning and LPC, as
 * lpcnet_synthesize_impl(..., N = 0) does; 0: into locals, as
 * run_frame_network_flush does (lpcnet.c:134-144) -- conv memories, the
 * lpc_from_cepstrum ring and frame_count advance, the conditioning and LPC
 * the next tail_impl reads stay. */
LPCNET_EXPORT int lpcnet_batch_run_frame_network(LPCNetBatch *b, const float *features, int update_conditions);

/* lpcnet_reset_signal (src/lpcnet.c:226-233) on one stream. */
LPCNET_EXPORT int lpcnet_batch_reset_signal(LPCNetBatch *b, int stream);

/* 1.6 kb/s decoder (lpcnet_decode, src/lpcnet.c:310-319): one 8-byte packet
 * per stream (decode_packet, lpcnet_dec.c:81-156, on the device) -> 4 frames
 * synthesised.  Needs a model blob with the codebook records
 * (LPCNetModelInfo.has_codebooks).  Each stream's vq_mem is part of its state
 * (reset to zero by lpcnet_batch_reset / _reset_stream, as
 * lpcnet_decoder_init does; saved and restored with it).
 * Host I/O: packets [B][8] -> pcm [B][4 * 160]. */
LPCNET_EXPORT int lpcnet_batch_decode(LPCNetBatch *b, const unsigned char *packets, short *pcm);
/* Device-resident: d_packets [npackets][B][8] -> d_pcm [4 npackets][B][160]
 * (the frames-major layout of lpcnet_batch_synthesize_frames); the decoded
 * features stay in device memory.  Enqueued; lpcnet_batch_sync waits. */
LPCNET_EXPORT int lpcnet_batch_decode_frames(LPCNetBatch *b, const unsigned char *d_packets, short *d_pcm, int npackets);

/* Snapshot / restore of one stream's complete synthesis state (the struct
 * copies lpcnet_plc.c:223,230 make for speculation).  buf holds
 * lpcnet_batch_state_size() bytes. */
LPCNET_EXPORT int lpcnet_batch_state_size(void);
LPCNET_EXPORT int lpcnet_batch_save_state(LPCNetBatch *b, int stream, void *buf);
LPCNET_EXPORT int lpcnet_batch_restore_state(LPCNetBatch *b, int stream, const void *buf);

/* nframes consecutive frames for every stream with device-resident I/O:
 * d_features [nframes][B][NB_FEATURES] and d_pcm [nframes][B][N] are device
 * pointers on the batch's device.  h_features is ignored (it may be NULL;
 * lpc_from_cepstrum runs on the device since round 2 -- kept for ABI
 * compatibility).  Work is enqueued on the batch's HIP stream; the call
 * returns once every frame has been enqueued (use lpcnet_batch_sync to wait). */
LPCNET_EXPORT int lpcnet_batch_synthesize_frames(LPCNetBatch *b, const float *h_features, const float *d_features,
                                                 short *d_pcm, int nframes, int N);
/* Wait for every enqueued frame.  Returns 0, or -1 (lpcnet_mi355x_last_error)
 * on a HIP error or a device-side abort (see lpcnet_batch_set_spin_limit). */
LPCNET_EXPORT int lpcnet_batch_sync(LPCNetBatch *b);

/* Bound on the polls of one LDS flag wait inside the barrier-free sample
 * kernel (fp_kernel).  A wait that exceeds it means a protocol fault: the
 * kernel finishes early instead of hanging the device, and the next
 * synchronising call (lpcnet_batch_synthesize / _impl / _sync) returns -1
 * with lpcnet_mi355x_last_error() set -- never silent wrong PCM.  0 restores
 * the default (2^20 polls); tiny values exist to test the reporting. */
LPCNET_EXPORT int lpcnet_batch_set_spin_limit(LPCNetBatch *b, int polls);

/* Multi-frame path for batches above 128 streams with the matrix-core or
 * fp32 sample kernel: the frame network of each run of up to 32 frames
 * (>= 4) is computed in one launch before their sample kernels (chunk_kernel,
 * f32 matrix cores; identical outputs).  enable = 0 selects the per-frame
 * frame kernel instead (A/B and parity tests); default 1. */
LPCNET_EXPORT int lpcnet_batch_set_frame_chunking(LPCNetBatch *b, int enable);

/* Device memory helpers (so callers need no HIP headers). */
LPCNET_EXPORT void *lpcnet_batch_device_alloc(LPCNetBatch *b, size_t bytes);
LPCNET_EXPORT int lpcnet_batch_device_free(LPCNetBatch *b, void *p);
LPCNET_EXPORT int lpcnet_batch_memcpy_h2d(LPCNetBatch *b, void *dst, const void *src, size_t bytes);
LPCNET_EXPORT int lpcnet_batch_memcpy_d2h(LPCNetBatch *b, void *dst, const void *src, size_t bytes);

/* Kernel timing (HIP events on the batch's stream, recorded around every
 * launch since the last reset_timers): which = 0 sample-network kernel,
 * 1 frame-network kernel (per-frame frame kernel, or chunk_kernel once per
 * run of frames), 2 the PLC predictor (lpcnet_batch_plc_predict*, timed
 * whenever enable > 0), 3 the feature extractor
 * (lpcnet_batch_compute_features*, one launch per frame, likewise), 4 the
 * 1.6 kb/s encoder (lpcnet_batch_encode*, lpcnet_batch_compute_features4:
 * the four analysis launches of a packet, one frame each, and the launches
 * of enc_kernel.hip as one region; likewise), 5 the part of 4 that is
 * enc_kernel.hip (four frames per region), 6 the Burg analysis kernel
 * (lpcnet_batch_burg_cepstrum*, _plc_rows_device with the Burg part,
 * _plc_update*: one launch per frame, timed whenever enable > 0; the rows'
 * extractor launch counts under 3, the update's predictor under 2), 8 the
 * RDO-VAE encoder and 9 the RDO-VAE decoder (lpcnet_batch_rdovae_*, timed
 * whenever enable > 0; a decode_all launch of n latents counts n frames).  7
 * is no region: -1, as every value outside the list.  Returns
 * total ms and the number of launches.
 * enable: 0 off, 1 events around the sample kernel only, 2 (or more) around
 * both kernels. */
LPCNET_EXPORT void lpcnet_batch_reset_timers(LPCNetBatch *b, int enable);
LPCNET_EXPORT double lpcnet_batch_kernel_ms(LPCNetBatch *b, int which, int *launches);
/* Frames covered by those timed launches (a multi-frame sample launch or a
 * chunk_kernel launch covers several). */
LPCNET_EXPORT int lpcnet_batch_kernel_frames(LPCNetBatch *b, int which);

/* Debug / parity: per-sample trace of the pre-sampling logits (8 per sample,
 * nnet.c:186-211) and the sampled excitation of the LAST synthesize call.
 * logits [B][N][8], exc [B][N]. */
LPCNET_EXPORT int lpcnet_batch_set_trace(LPCNetBatch *b, int enable);
LPCNET_EXPORT int lpcnet_batch_get_trace(LPCNetBatch *b, float *logits, int *exc);
/* Diagnostics: per-phase s_memtime sums of the sample kernel, recorded for
 * the LAST launch when enabled: [workgroup][8 waves][16] u64 (phase B, wait,
 * phase C, wait, phase F, wait, loop total, samples, then F sub-phases:
 * GRU_B update, broadcast, tree levels 0-3, levels 4-7, output; the
 * pipelined kernel records [0] X->Y work, [1] wait, [2] Y->Z work, [3] wait,
 * [4] Z->X work, [5] wait per wave).  Returns #workgroups. */
LPCNET_EXPORT int lpcnet_batch_set_stamps(LPCNetBatch *b, int enable);
LPCNET_EXPORT int lpcnet_batch_get_stamps(LPCNetBatch *b, unsigned long long *out);
/* Frame-kernel phase stamps of the last launch: [B/4 workgroups][16]
 * (0 prologue, 1 conv1, 2 conv2, 3 dense1, 4 dense2, 5 projections,
 * 6 epilogue, 7 total), cycles. */
LPCNET_EXPORT int lpcnet_batch_get_frame_stamps(LPCNetBatch *b, unsigned long long *out);

/* Per-stream state snapshot: any pointer may be NULL. */
LPCNET_EXPORT int lpcnet_batch_get_state(LPCNetBatch *b, int stream, float *gru_a_cond /*1152*/, float *gru_b_cond /*48*/,
                                         float *lpc /*16*/, float *gru_a_state /*384*/, float *gru_b_state /*16*/,
                                         int *frame_count);

/* ---- tooling (host only, no GPU needed) -------------------------------- */
/* Deterministic synthetic default-size model in the reference blob format.
 * flags: bit0 = make some int8 pairs able to saturate maddubs; bit1 = GRU_A
 * block masks chosen as training_tf2/lpcnet.py:140-160 (Sparsify) does --
 * a global per-gate energy threshold -- over skewed row energies, so block
 * rows run far above the mean length, as in trained models; bit2 = append
 * synthetic 1.6 kb/s decoder codebooks (ceps_codebook1..3 [1024][17],
 * ceps_codebook_diff4 [4096][18]; the other arrays are unchanged); bit3 =
 * append the PLC prediction network's records (training_tf2/dump_plc.py) in
 * the reference's default shape (cond 128, two GRUs of 256 units,
 * lpcnet_plc.py:94-103), non-saturating; bits 3 and 4 = the same in a small
 * unequal shape (cond 64, 128 and 64 units); without bit3 the blob is
 * unchanged; bit5 = append the DRED RDO-VAE's records
 * (training_tf2/dump_rdovae.py), encoder and decoder, in the default shape
 * (every stack layer 256 wide, T = 2048, gdense1 128, 80 latents, a 24-value
 * state, conv kernel 4), non-saturating; bits 5 and 6 = the same in a small
 * unequal shape (dense1/3/5 128 wide, the GRUs and dense7/8 64, T = 704,
 * gdense1 64, 40 latents, a 32-value state); without bit5 the blob is
 * unchanged.
 * Returns the blob size; writes it if buf != NULL and cap is large enough. */
LPCNET_EXPORT int lpcnet_mi355x_synthetic_model(unsigned seed, int variant, int flags, unsigned char *buf, int cap);
/* Synthetic feature frames (NB_TOTAL_FEATURES floats each) for stream `stream`. */
LPCNET_EXPORT void lpcnet_mi355x_synthetic_features(unsigned stream, int nframes, float *out);
/* lpc_from_cepstrum (freq.c:310-320) of n cepstra [n][18] -> lpc [n][16] on
 * GPU `device`, through the engine's lpc_kernel (diagnostics / parity: the
 * synthesis entry points run the same kernel per frame).  Returns 0 or -1. */
LPCNET_EXPORT int lpcnet_mi355x_device_lpc(int device, const float *cepstra, float *lpc, int n);
/* The rcpps table the device activations use by default (2048 entries:
 * the Intel build host's rcpps of the top 11 mantissa bits,
 * tests/golden/rcp_x86.bin). */
LPCNET_EXPORT const uint32_t *lpcnet_mi355x_rcp_table(void);
/* This host CPU's rcpps (_mm_rcp_ps, vec_avx.h:408,437) of every float in
 * [1, 2) as 4096 entries of the top 12 mantissa bits (entries == 4096).
 * Returns the number of mantissas / exponents the 12-bit, exponent-invariant
 * form does not reproduce (0: the table is exact), or -1. */
LPCNET_EXPORT int lpcnet_mi355x_host_rcp_table(uint32_t *tab, int entries);
/* Same-box parity: the device activations use rcpps table `tab` (4096
 * entries as lpcnet_mi355x_host_rcp_table returns; NULL restores the
 * default Intel table).  A table other than the default disables the
 * hardware-reciprocal shortcut (proven equal only to the Intel table), so
 * the batch runs the lockstep sample kernel and the per-frame frame kernel
 * (every activation through the table).  The environment variable
 * LPCNET_RCP=host selects this host's table at load time (drop-in API).
 * Returns 0, or -1 (no model loaded / device error). */
LPCNET_EXPORT int lpcnet_batch_set_rcp_table(LPCNetBatch *b, const uint32_t *tab);
/* Device numerics self-test (diagnostics, not the synthesis path): runs one
 * routine of the kernels' arithmetic (lpcnet_amd/csrc/device_math.h) on GPU
 * `device` elementwise over n 32-bit inputs: op 0 tanh8_approx, 1
 * sigmoid8_approx (vec_avx.h:393-440, rcpps from the table), 2 / 3 the
 * batched forms of 0 / 1 with the hardware rcpps form, 4 vector_ps_to_epi8 byte (vec_avx.h:321-336), 5 lin2ulaw
 * (common.h:47-58), 6 floor(.5 + x) (lpcnet.c:266), 7 _mm256_cvtps_epi32;
 * op 8: n kiss99 draws (kiss99.c:59-81) from the 4-word state in[0..3];
 * op 9: the band power of lpc_from_cepstrum, (float)(pow(10, x) *
 * compensation[i % 18]) (freq.c:318, pow10_dd.h); op 10 _mm256_rcp_ps of a
 * Pade denominator (vec_avx.h:408,437, hardware form); op 11 / 12
 * sigmoid8_approx of the int8 gates' inputs (|x| < 2^18, device_math.h
 * sigmoid_x86_fin_n), hardware / table rcpps; op 13 / 14 tanh8_approx in its
 * select-free form (finite |x| < 2^30, device_math.h tanh_x86_fin_n),
 * hardware / table rcpps.
 * Returns 0, or -1 on bad arguments / HIP failure. */
LPCNET_EXPORT int lpcnet_mi355x_device_numerics(int device, int op, const void *in, void *out, int n);
/* Validate a weight blob with every rule lpcnet_load_model applies
 * (parse_lpcnet_weights.c:36-113 record/idx rules, array sizes, LDS budget)
 * without a device.  Returns 0 or -1 (lpcnet_mi355x_last_error). */
LPCNET_EXPORT int lpcnet_mi355x_validate_model(const unsigned char *data, int len);
/* Host-only digests of everything a load of the blob would hand a batch of
 * `streams` streams: one FNV-1a-64 per entry, in this order:
 *   [0]      the sample kernels' scalars of every family (their table
 *            offsets, group counts, bounds and forms) as one block;
 *   [1..56]  the device tables, as uploaded: the frame network's conv1_w,
 *            conv1_b, conv2_w, conv2_b, dense1_w, dense1_b, dense2_w,
 *            dense2_b, gadf_w, gadf_b, gbdf_w, gbdf_b, proj_w, proj_b,
 *            ck_conv1, ck_conv2, ck_dense1, ck_dense2, ck_proj, embed_pitch,
 *            rcp; the sample kernels' emb_sig, emb_pred, emb_exc, ga_par,
 *            ga_wsum, gb_par, gb_wsum, image, mf, mf_unit, mf_frow, mfw_tab,
 *            mfw_frow, mfw_unit, mf_emb[0..2], mfw_emb[0..2], mf_gb, fp_zr,
 *            fp_h, fp_off, fpl_zr, fpl_h, fpl_off, fp_gb, ga_wf, gb_recf; the
 *            decoder's cb1, cb2, cb3, cbd, pitch (0: the model has no such
 *            table);
 *   [57]     the chunk kernel's four replication strides;
 *   [58]     variant, may-saturate, quad layout, matrix-core / fp32-kernel
 *            tables present, codebooks, wide plan, custom rcpps, the lockstep
 *            kernel's streams per workgroup and LDS bytes, GRU_A and GRU_B
 *            block counts (ints);
 *   [59]     bytes_shared_per_frame, bytes_shared_per_sample,
 *            bytes_per_stream_sample, ops_per_sample, the matrix-core GRU_A
 *            and GRU_B ops per group and sample (doubles).
 * wide: 1 / 0 = the register tables are planned for mfw_kernel or not; -1 =
 * as a batch on a device of `cus` compute units decides.  Returns the number
 * of entries written (60; cap must hold them) or -1. */
LPCNET_EXPORT int lpcnet_mi355x_model_digest(const unsigned char *data, int len, int streams, int cus, int wide, uint64_t *out,
                                             int cap);
/* Host-only digests of the tables beside the synthesis model, one FNV-1a-64
 * per entry:
 *   [0..9]   the PLC predictor's device tables, as uploaded: d1_w, d1_b,
 *            g1_in, g1_rec, g1_seed, g2_in, g2_rec, g2_seed, out_w, out_b
 *            (0 each when data is NULL or the blob has no usable PLC records);
 *   [10]     the lpc_from_cepstrum tables (lpc_kernel.hip);
 *   [11]     the feature extractor's tables (feat_kernel.hip);
 *   [12..15] not digests: the PLC dims as lpcnet_mi355x_plc_dims gives them
 *            (0 each without usable PLC records).
 * Returns the number of entries written (16; cap must hold them) or -1. */
LPCNET_EXPORT int lpcnet_mi355x_side_digest(const unsigned char *data, int len, uint64_t *out, int cap);
/* Host-only: which sample kernel and which frame path a batch of `streams`
 * streams of the blob takes on a device of `cus` compute units (0: as many
 * as the current HIP device has, the only case that asks a device), with
 * `kernel_mode` (lpcnet_batch_set_kernel), a custom rcpps table or not, and
 * the current environment (LPCNET_MF2, LPCNET_MFW, LPCNET_MFW_G,
 * LPCNET_NO_CHUNK, LPCNET_NO_MULTIFRAME, LPCNET_NO_OVERLAP, LPCNET_LPC_EAGER,
 * LPCNET_NO_DIRECT_PCM).  The host model is built as a load builds it.
 *   plan[LPCNET_CHOICE_PLAN]: base kernel (0 lockstep sample_kernel, 1
 *     mf_kernel, 4 fp_kernel), mf2, mfw, mfw_g, mfw_forced, plan_wide (the
 *     plan class the register tables were built for), rcp_hw, then
 *     LPCNetModelInfo's quad_path, streams_per_workgroup, lds_bytes and
 *     mfma_ops_per_group_sample (as an integer), then whether the batch-level
 *     predicate asks for the wide plan class and whether the model has
 *     matrix-core tables at all (only then does a batch re-plan);
 *   launches [nlaunches][4] = (streams of the launch, preload, trace,
 *     stamps) -> launch_out [nlaunches][2] = (kernel: 0 lockstep, 1
 *     mf_kernel, 2 mf2_kernel, 3 mfw_kernel, 4 fp_kernel; its PCM store is
 *     coalesced, so a host-I/O tick may store PCM straight to host memory);
 *   calls [ncalls][10] = (nframes, N, streams of the call, preload, frame
 *     chunking, the batch has a second queue, trace, stamps, features_delay,
 *     end2end) -> call_out [ncalls][5] = (lpcnet_batch_synthesize_frames:
 *     multi-frame sample launches, overlapped frame kernels, chunked frame
 *     network; lpcnet_batch_synthesize: the one-frame chunked form, deferred
 *     LPC).
 * Returns the CU count planned for, or -1 (lpcnet_mi355x_last_error). */
#define LPCNET_CHOICE_PLAN 13
LPCNET_EXPORT int lpcnet_mi355x_kernel_choice(const unsigned char *data, int len, int streams, int cus, int kernel_mode,
                                              int rcp_custom, int *plan, const int *launches, int nlaunches, int *launch_out,
                                              const int *calls, int ncalls, int *call_out);
/* Number of visible HIP devices (0 on a machine without GPU). */
LPCNET_EXPORT int lpcnet_mi355x_device_count(void);
/* Host-only view of the GRU_A plans a blob (data, len) gets on a wide batch
 * (no device touched): out[0] = split model (0/1), out[1] = mfw_kernel's
 * split form available (0/1), out[2 + 2w], out[3 + 2w] = its z/r and h
 * 4-slot groups of table wave w (R waves 0..5, host waves 6..7),
 * out[18..20] = pieces per gate.  int out[24].  0 / -1. */
LPCNET_EXPORT int lpcnet_mi355x_wide_plan(const unsigned char *data, int len, int *out);
/* The drop-in handles (include/lpcnet.h) bound to the same model on the
 * same device share one device copy of it and one work batch; concurrent
 * lpcnet_synthesize calls on them coalesce into one launch.  Statistics of
 * the pool `st` belongs to: coalesced launches, handled requests, handles
 * bound.  -1 if st is not bound. */
LPCNET_EXPORT int lpcnet_mi355x_pool_stats(const LPCNetState *st, long *launches, long *requests, int *streams);
/* Placement of drop-in handles (lpcnet_init / lpcnet_create /
 * lpcnet_decoder_init take no device, lpcnet.c:184-219).  Default: every
 * handle on one device -- LOCAL_RANK mod the visible devices when LOCAL_RANK
 * is set (one process per GPU), device 0 otherwise -- resolved at the first
 * lpcnet_load_model, so creating handles never starts the HIP runtime.
 * Spreading is opt-in: over `devices[0..n)` here, or over env
 * LPCNET_DEVICES="0,1,..." / "all" (checked against the visible devices at
 * the first lpcnet_init: a bad list fails it), each new handle goes to the
 * placement with the fewest live handles (a device may appear twice: two
 * placements, two pools on one GPU).  Live handles keep their device;
 * handles initialised afterwards are placed over the new list; n = 0
 * restores the default.  LPCNET_DEVICE=d pins every new handle to device d
 * instead.  0 / -1. */
LPCNET_EXPORT int lpcnet_mi355x_set_placement(const int *devices, int n);
/* The device and placement index (-1: pinned by LPCNET_DEVICE) of handle st. */
LPCNET_EXPORT int lpcnet_mi355x_handle_placement(const LPCNetState *st, int *device, int *placement);
/* Milliseconds the pool of `st` has spent inside its coalesced launches
 * (host I/O, state moves and kernels of each launch; the rest of a caller's
 * wait is hand-off and thread wake-up).  -1 if st is not bound. */
LPCNET_EXPORT double lpcnet_mi355x_pool_run_ms(const LPCNetState *st);
/* ---- reference-internal entry points on a drop-in handle ----------------
 * The reference's PLC (lpcnet_plc.c:188-337) drives one LPCNetState through
 * these functions of lpcnet_private.h:126-132; they are exported here under
 * the same names and signatures so that code links against this library
 * unchanged, except for its LPCNetState struct copies (lpcnet_plc.c:223,230),
 * which become lpcnet_mi355x_state_save / _restore. */
LPCNET_EXPORT void lpcnet_synthesize_impl(LPCNetState *st, const float *features, short *output, int N, int preload);
LPCNET_EXPORT void lpcnet_synthesize_tail_impl(LPCNetState *st, short *output, int N, int preload);
LPCNET_EXPORT void run_frame_network_deferred(LPCNetState *st, const float *features);
LPCNET_EXPORT void run_frame_network_flush(LPCNetState *st);
LPCNET_EXPORT void lpcnet_reset_signal(LPCNetState *st);
/* A handle's whole synthesis state (device stream state + the deferred
 * feature buffer): buf holds lpcnet_mi355x_state_size() bytes.  Restore
 * refuses a buffer this engine cannot have produced.  0 / -1. */
#define LPCNET_MI355X_STATE_MAX 16384 /* >= lpcnet_mi355x_state_size() (stack buffers) */
LPCNET_EXPORT int lpcnet_mi355x_state_size(void);
LPCNET_EXPORT int lpcnet_mi355x_state_save(LPCNetState *st, void *buf);
LPCNET_EXPORT int lpcnet_mi355x_state_restore(LPCNetState *st, const void *buf);
/* Release what lpcnet_init bound to st without freeing st: for an
 * LPCNetState embedded in a caller's struct (as lpcnet_plc.c:63 / lpcnet.c:293
 * embed theirs) that the caller frees itself.  Memory freed without it is
 * detected as stale by the next lpcnet_init at that address. */
LPCNET_EXPORT void lpcnet_mi355x_deinit(LPCNetState *st);
/* Bind a model to a decoder (the reference binds its compiled-in model and
 * codebooks in lpcnet_decoder_init; this library has none).  -1 if the blob
 * is rejected or carries no codebooks. */
LPCNET_EXPORT int lpcnet_mi355x_decoder_load_model(LPCNetDecState *st, const unsigned char *data, int len);

/* ---- PLC prediction network (compute_plc_pred, lpcnet_plc.c:135-145) ------
 * The network that predicts the features of a lost frame -- plc_dense1 (57 ->
 * cond, tanh), plc_gru1 and plc_gru2 (compute_gruB), plc_out (-> NB_FEATURES)
 * and out[19] = min(.5, out[19] + .1) -- for every stream of a batch in one
 * launch (plc_kernel.hip), bit-identical per stream to the reference's AVX2
 * DOT_PROD build.  Its records (training_tf2/dump_plc.py: plc_dense1_weights
 * / _bias, plc_gru{1,2}_weights / _weights_idx / _recurrent_weights / _bias /
 * _subias, plc_out_weights / _bias) are optional in a blob, like the decoder
 * codebooks; the dimensions come from the record sizes (cond, units1, units2:
 * multiples of 64 up to 512).  A blob without usable records synthesises as
 * ever and these calls return -1 with the reason in
 * lpcnet_mi355x_last_error: missing or mis-sized records, unsupported
 * dimensions, an fp32 (LPCNET_VARIANT_FP32) blob, int8 weights in which a
 * maddubs pair can saturate.  Emulating that saturation (trained PLC models
 * are clipped against it, lpcnet_plc.py:69-91) and an fp32 predictor are out
 * of scope.  Each stream's predictor state (plc_gru1_state, plc_gru2_state:
 * PLCNetState) lives beside its synthesis state, not in it:
 * lpcnet_batch_state_size and the synthesis snapshots are unchanged;
 * lpcnet_batch_reset / _reset_stream zero it (lpcnet_plc_reset). */
/* dims[4] = {57, cond, units1, units2}; -1 (last_error) if the blob has no usable PLC records. Host only. */
LPCNET_EXPORT int lpcnet_mi355x_plc_dims(const unsigned char *data, int len, int dims[4]);
LPCNET_EXPORT int lpcnet_batch_plc_info(const LPCNetBatch *b, int dims[4]);
/* compute_plc_pred for every stream s with active[s] != 0 (active == NULL: all).
 * in [B][57] (NULL: all-zero input, the concealment call lpcnet_plc.c:161-162);
 * out [B][NB_FEATURES] (NULL: discard, :158). Inactive streams: state and out row untouched. */
LPCNET_EXPORT int lpcnet_batch_plc_predict(LPCNetBatch *b, const float *in, float *out, const unsigned char *active);
/* the same with device pointers, enqueued on the batch's stream (lpcnet_batch_sync waits);
 * d_out has the [B][NB_FEATURES] layout lpcnet_batch_synthesize_frames reads as d_features */
LPCNET_EXPORT int lpcnet_batch_plc_predict_device(LPCNetBatch *b, const float *d_in, float *d_out, const unsigned char *d_active);
LPCNET_EXPORT int lpcnet_batch_plc_reset(LPCNetBatch *b, int stream /* -1: all */);
/* PLCNetState copies (plc_copy[], lpcnet_plc.c:217, 233, 305-306, 313-314) */
LPCNET_EXPORT int lpcnet_batch_plc_state_size(const LPCNetBatch *b);
LPCNET_EXPORT int lpcnet_batch_plc_save_state(LPCNetBatch *b, int stream, void *buf);
LPCNET_EXPORT int lpcnet_batch_plc_restore_state(LPCNetBatch *b, int stream, const void *buf);

/* ---- Feature extraction (lpcnet_compute_single_frame_features) -------------
 * The analysis side for a whole batch in one launch per frame
 * (feat_kernel.hip): preemphasis, compute_frame_features and
 * process_single_frame (lpcnet_enc.c:872-880, 488-577, 814-870, pcount = 0),
 * what lpcnet_plc_update_causal / _conceal_causal run on every frame
 * (lpcnet_plc.c:251-254, 322-328), bit-identical per stream to the
 * reference's build.  A row of NB_TOTAL_FEATURES (36) floats per stream:
 * [0, 18) the cepstrum, [18] the pitch, [19] the pitch correlation, [20, 36)
 * the frame's LPC.  The analysis has no weights: these calls need no model
 * and no call that changes the model or its kernels changes their results.
 * Each stream's analysis state (the part of LPCNetEncState this path carries)
 * lives beside its synthesis state, not in it, and is allocated by the first
 * of these calls: lpcnet_batch_state_size and the synthesis snapshots are
 * unchanged; lpcnet_batch_reset / _reset_stream zero it (lpcnet_encoder_init
 * inside lpcnet_plc_reset).
 * burg_cepstral_analysis and the predictor's input rows are the section
 * "Burg cepstral analysis" below.
 * The PLC state machine over these calls is the section "Concealment
 * machine" below.  Out of scope: process_multi_frame and drop-in
 * LPCNetEncState handles (one stream per launch is slower than the CPU).
 * Argument errors return -1 with the reason in lpcnet_mi355x_last_error. */
/* lpcnet_compute_single_frame_features for every stream s with active[s] != 0
 * (NULL: all). pcm [B][160]; features [B][NB_TOTAL_FEATURES]. Inactive streams:
 * state and output row untouched. */
LPCNET_EXPORT int lpcnet_batch_compute_features(LPCNetBatch *b, const short *pcm, float *features, const unsigned char *active);
LPCNET_EXPORT int lpcnet_batch_compute_features_float(LPCNetBatch *b, const float *pcm, float *features,
                                                      const unsigned char *active);
/* device pointers, enqueued on the batch's stream (lpcnet_batch_sync waits):
 * nframes consecutive frames, d_pcm [nframes][B][160] (the layout
 * lpcnet_batch_synthesize_frames writes), d_features [nframes][B][row] with
 * row = NB_FEATURES (what synthesize_frames reads as d_features; columns
 * 36..55 of a plc_predict_device input row hold the same 20 values) or
 * NB_TOTAL_FEATURES; anything else -1.  d_active [B] applies to every frame. */
LPCNET_EXPORT int lpcnet_batch_compute_features_device(LPCNetBatch *b, const short *d_pcm, float *d_features, int row,
                                                       const unsigned char *d_active, int nframes);
LPCNET_EXPORT int lpcnet_batch_features_reset(LPCNetBatch *b, int stream /* -1: all */);
/* snapshots of one stream's analysis state; the size is the same for every batch (b may be NULL) */
LPCNET_EXPORT int lpcnet_batch_features_state_size(const LPCNetBatch *b);
LPCNET_EXPORT int lpcnet_batch_features_save_state(LPCNetBatch *b, int stream, void *buf);
LPCNET_EXPORT int lpcnet_batch_features_restore_state(LPCNetBatch *b, int stream, const void *buf);

/* ---- Burg cepstral analysis and the predictor's input rows -----------------
 * burg_cepstral_analysis (freq.c:156-199, burg.c:98-245) for a whole batch in
 * one launch per frame (burg_kernel.hip): 160 samples per stream -> 36 floats,
 * the 18 half-sums and 18 differences of the two half-frames' Burg cepstra,
 * bit-identical per stream to the reference's build (-ffp-contract=off, no
 * fast-math).  It has no state across frames and no weights: these calls need
 * no model, and no call that changes the model or its kernels changes their
 * results.  Inputs on which the reference build aborts (the asserts of
 * silk_burg_analysis: nrg_f > 0, nrg_b > 0, |rc| < 1) are outside the
 * contract.
 * With it every per-frame step of lpcnet_plc_update_causal / _non_causal
 * (lpcnet_plc.c:205-258, 374-436) is a batch call: plc_rows assembles the
 * predictor's input row [36 Burg cepstrum | 20 features | flag] in device
 * memory, plc_update is rows + compute_plc_pred, the good-packet step.
 * The PLC state machine itself (pcm_fill loops, blending, DC filter, FEC
 * queue) is the section "Concealment machine" below.  Out of scope:
 * process_multi_frame and an fp32 predictor.
 * Argument errors return -1 with the reason in lpcnet_mi355x_last_error and
 * launch nothing. */
/* burg_cepstral_analysis for every stream s with active[s] != 0 (NULL: all).
 * pcm [B][160]; ceps [B][36]. Inactive streams: output row untouched. */
LPCNET_EXPORT int lpcnet_batch_burg_cepstrum(LPCNetBatch *b, const short *pcm, float *ceps, const unsigned char *active);
LPCNET_EXPORT int lpcnet_batch_burg_cepstrum_float(LPCNetBatch *b, const float *pcm, float *ceps, const unsigned char *active);
/* device pointers, on the batch's stream: d_pcm [nframes][B][160] (what
 * synthesize_frames writes); the 36 values go to d_out[(f*B + s)*row + col .. +36);
 * row >= col + 36, col >= 0, anything else -1; other columns untouched. */
LPCNET_EXPORT int lpcnet_batch_burg_cepstrum_device(LPCNetBatch *b, const short *d_pcm, float *d_out, int row, int col,
                                                    const unsigned char *d_active, int nframes);

#define LPCNET_PLC_ROW_BURG     1  /* columns 0..35 = burg_cepstral_analysis(d_pcm) */
#define LPCNET_PLC_ROW_FEATURES 2  /* columns 36..55 = the extractor's first 20 features of d_pcm; advances the analysis state */
/* One predictor input row [B][57] per active stream: the selected parts,
 * zeros in an unselected part, `flag` in column 56 (lpcnet_plc.c:212-214,
 * 256-257, 380-382, 434-435). d_pcm [B][160]. Inactive streams: row and state
 * untouched. parts outside 1..3: -1. */
LPCNET_EXPORT int lpcnet_batch_plc_rows_device(LPCNetBatch *b, const short *d_pcm, float *d_rows, int parts, float flag,
                                               const unsigned char *d_active);
/* The good-packet step: rows(BURG|FEATURES, flag 1) then compute_plc_pred;
 * pcm / d_pcm [B][160], out / d_out [B][NB_FEATURES], neither NULL.  Needs a
 * model with PLC records. */
LPCNET_EXPORT int lpcnet_batch_plc_update(LPCNetBatch *b, const short *pcm, float *out, const unsigned char *active);
LPCNET_EXPORT int lpcnet_batch_plc_update_device(LPCNetBatch *b, const short *d_pcm, float *d_out, const unsigned char *d_active);

/* ---- 1.6 kb/s encoder (lpcnet_encode, lpcnet_compute_features) -------------
 * lpcnet_enc.c:882-909 for a whole batch: four analysis launches
 * (feat_kernel.hip's superframe form) and process_superframe
 * (enc_kernel.hip), bit-identical per stream to the reference's build with
 * quantize = encode = 1 (lpcnet_encode) or 0 (lpcnet_compute_features).  A
 * stream's encoder state is its analysis state above (the Viterbi rows are
 * the single-frame path's: single-frame and four-frame calls on one stream
 * behave as one LPCNetEncState does) plus the encoder's own vq_mem[18], which
 * is not the decoder's; lpcnet_batch_reset, _reset_stream and
 * _features_reset zero both.  Codebook distances of 1e15f or more, and NaN,
 * are outside the contract (the reference then reads uninitialised indices);
 * PCM input cannot produce them.  Inactive streams keep their state, packet
 * and feature rows. */
/* lpcnet_encode: pcm [B][640] -> packets [B][8]; features (NULL: not wanted)
 * [4][B][NB_TOTAL_FEATURES] receives st->features after quantisation, what a
 * decoder reconstructs plus its LPC.  Needs a model with the ceps codebooks. */
LPCNET_EXPORT int lpcnet_batch_encode(LPCNetBatch *b, const short *pcm, unsigned char *packets, float *features,
                                      const unsigned char *active);
/* lpcnet_compute_features: unquantised; pcm [B][640] -> features
 * [4][B][NB_TOTAL_FEATURES].  Needs no model. */
LPCNET_EXPORT int lpcnet_batch_compute_features4(LPCNetBatch *b, const short *pcm, float *features, const unsigned char *active);
/* device pointers, enqueued on the batch's stream: d_pcm [4 npackets][B][160]
 * (what lpcnet_batch_synthesize_frames writes), d_packets [npackets][B][8]
 * (what lpcnet_batch_decode_frames reads), d_features (NULL: not wanted)
 * [4 npackets][B][row], row NB_FEATURES or NB_TOTAL_FEATURES; anything else -1. */
LPCNET_EXPORT int lpcnet_batch_encode_device(LPCNetBatch *b, const short *d_pcm, unsigned char *d_packets, float *d_features,
                                             int row, const unsigned char *d_active, int npackets);
/* snapshots of one stream's encoder state: the features snapshot followed by vq_mem[18] */
LPCNET_EXPORT int lpcnet_batch_encode_state_size(const LPCNetBatch *b);
LPCNET_EXPORT int lpcnet_batch_encode_save_state(LPCNetBatch *b, int stream, void *buf);
LPCNET_EXPORT int lpcnet_batch_encode_restore_state(LPCNetBatch *b, int stream, const void *buf);
/* Host only: main_pitch of lpcnet_enc.c:678-679 for n values of center_pitch,
 * from the threshold table the encoder kernel uses (the smallest float that
 * reaches each main_pitch under the host's double log) and evaluated as the
 * kernel evaluates it.  Non-finite and non-positive inputs give 0, as the
 * x86 (int) cast does. */
LPCNET_EXPORT int lpcnet_mi355x_enc_main_pitch(const float *center_pitch, int *out, int n);

/* ---- Concealment machine (lpcnet_plc_update / lpcnet_plc_conceal) -----------
 * lpcnet_plc.c:188-503 for a whole batch, one call per 10 ms tick, in the
 * reference's three modes (causal, non-causal, codec):
 * every stream s has the semantics of one reference LPCNetPLCState (built, as
 * the reference ships, with PLC_SKIP_UPDATES defined), bit-identical in the
 * PCM of every tick and in its state to the same stream run alone.  Streams
 * that received their packet and streams that lost it share the call.  The
 * control state (pcm_fill, skip_analysis, blend, loss_count, the FEC queue's
 * positions, the deferred-feature fill, queued_update) depends on the sequence of lost and
 * received ticks and FEC adds alone, so the host plans a tick for every stream
 * without reading anything back; all of a tick's work is queued on the
 * batch's stream and nothing synchronises between its steps.  The machine's
 * per-stream data (st->features, st->pcm, dc_mem / syn_dc, plc_copy, the FEC
 * queue, the deferred features) lives beside the synthesis state:
 * lpcnet_batch_state_size and the snapshots are unchanged.  The synthesis,
 * predictor and analysis state the machine advances are the batch's own
 * (lpcnet_batch_save_state, _plc_save_state, _features_save_state see them).
 * FEATURES_DELAY is the batch's at the time of the open; a tick after
 * lpcnet_batch_set_model_constants changed it is refused (close and reopen).
 * lpcnet_batch_load_model closes the machine.  lpcnet_batch_reset /
 * _reset_stream also reset the machine's streams.
 * The non-causal mode (lpcnet_plc.c:339-492) delays its output by 80 samples
 * and, on the first received tick after a loss, synthesises backwards over
 * the received frame to cross-fade into it.  Like the reference it exists
 * only for models with FEATURES_DELAY 0 (the reference exits otherwise,
 * :357-361): an open on a batch with another delay is refused.  Its control
 * state is loss_count and queued_update alone; it never reads the FEC queue,
 * though fec_add / fec_clear still move the queue's positions.  Every received
 * tick runs a full 160-sample teacher-forced synthesis (this branch has no
 * PLC_SKIP_UPDATES shortcut); the first received tick after a loss runs 320
 * speculative samples and queues 160 more for the next tick.  Its extra
 * per-stream data (queued_samples, dc_buf, the saved synthesis state) is
 * allocated by the open of that mode only.
 * Out of scope: the #else branches of PLC_SKIP_UPDATES, the disabled
 * alternative of :419-422, an fp32 predictor, drop-in LPCNetPLCState
 * handles.  Received frames on which burg_cepstral_analysis aborts in the
 * reference (all-zero half-frames) are outside the contract, as above.
 * Every refusal returns -1 with the reason in lpcnet_mi355x_last_error and
 * launches nothing. */
#define LPCNET_CONCEAL_CAUSAL    0 /* the values of the reference's LPCNET_PLC_* */
#define LPCNET_CONCEAL_NONCAUSAL 1 /* FEATURES_DELAY 0 only */
#define LPCNET_CONCEAL_CODEC     2
#define LPCNET_CONCEAL_DC_FILTER 4
/* lpcnet_plc_init + lpcnet_plc_reset for every stream (the synthesis,
 * predictor and analysis states are reset too).  Needs a model with usable PLC
 * records; one machine per batch.  LPCNET_CONCEAL_NONCAUSAL on a batch whose
 * FEATURES_DELAY is not 0: -1, "non-causal ... FEATURES_DELAY". */
LPCNET_EXPORT int lpcnet_batch_conceal_open(LPCNetBatch *b, int options);
LPCNET_EXPORT int lpcnet_batch_conceal_close(LPCNetBatch *b);
LPCNET_EXPORT int lpcnet_batch_conceal_reset(LPCNetBatch *b, int stream /* lpcnet_plc_reset; -1: all */);
/* One tick: stream s with lost[s] == 0 runs lpcnet_plc_update on pcm[s]
 * (in/out), with lost[s] != 0 lpcnet_plc_conceal into pcm[s] (out);
 * active[s] == 0 (NULL: all active): no tick for s, row and state untouched.
 * pcm [B][160], lost [B]. */
LPCNET_EXPORT int lpcnet_batch_conceal_frame(LPCNetBatch *b, short *pcm, const unsigned char *lost, const unsigned char *active);
/* the same on device PCM [B][160], queued (lpcnet_batch_sync waits); lost and
 * active are host memory, read during the call */
LPCNET_EXPORT int lpcnet_batch_conceal_frame_device(LPCNetBatch *b, short *d_pcm, const unsigned char *lost,
                                                    const unsigned char *active);
/* lpcnet_plc_fec_add (features [20]; NULL: fec_skip++) and lpcnet_plc_fec_clear
 * on one stream.  An add into a full queue with nothing to drop returns -1,
 * "FEC buffer full", the state unchanged (the reference prints and returns). */
LPCNET_EXPORT int lpcnet_batch_conceal_fec_add(LPCNetBatch *b, int stream, const float *features);
LPCNET_EXPORT int lpcnet_batch_conceal_fec_clear(LPCNetBatch *b, int stream);
/* tests / diagnostics, after a synchronisation: ctrl [9] = pcm_fill,
 * skip_analysis, blend, loss_count, fec_fill_pos, fec_read_pos, fec_keep_pos,
 * fec_skip, feature_buffer_fill; features [20] = st->features; pcm_buf
 * [FEATURES_DELAY * 160 + 240] = st->pcm; dc [2] = dc_mem, syn_dc */
LPCNET_EXPORT int lpcnet_batch_conceal_get_state(LPCNetBatch *b, int stream, int *ctrl, float *features, short *pcm_buf, double *dc);
/* the non-causal mode's own state, after a synchronisation; any pointer may be
 * NULL: queued_update, queued_samples [160], dc_buf [80].  -1 when the open
 * machine is in another mode. */
LPCNET_EXPORT int lpcnet_batch_conceal_get_state_noncausal(LPCNetBatch *b, int stream, int *queued_update, short *queued_samples,
                                                           short *dc_buf);
/* Host only: the machine's planner on one stream from reset over nticks ticks.
 * lost [nticks]; fec_adds [nticks] (NULL: none): before tick t, n > 0 adds,
 * -1 a NULL add, -2 a clear.  steps (NULL: count only) receives up to
 * max_steps triples (op, a, b) -- the primitive calls of lpcnet_plc.c in order,
 * see conceal_plan.h -- tick_end [nticks] (NULL: not wanted) the number of
 * steps up to and including each tick, ctrl [nticks][9] (NULL: not wanted) the
 * control fields after each tick.  Returns the number of steps.  The non-causal
 * mode at a features_delay other than 0 is refused as the open refuses it. */
LPCNET_EXPORT int lpcnet_mi355x_conceal_plan(int options, int features_delay, const unsigned char *lost, const int *fec_adds,
                                             int nticks, int *steps, int max_steps, int *tick_end, int *ctrl);

/* ---- DRED RDO-VAE (dred_rdovae_enc.c, dred_rdovae_dec.c, dred_rdovae.c) -----
 * The redundancy codec's networks for a whole batch, one launch per call
 * (rdovae_kernel.hip), bit-identical per stream to the reference's x86
 * DOT_PROD build.  The encoder turns two consecutive 20-feature frames (the
 * earlier first) into L latents and an S-value initial state
 * (dred_rdovae_encode_dframe); the decoder turns an initial state and
 * latents back into feature frames, four per latent in the reference's
 * reverse order (dec_init_states, decode_qframe, DRED_rdovae_decode_all).
 * The records are optional in a blob and come from
 * training_tf2/dump_rdovae.py: enc_dense1..8, bits_dense, gdense1, gdense2
 * for the encoder, state1..3, dec_dense1..8, dec_final for the decoder; the
 * two sides are independent, a blob may carry either, both or neither.
 * Every dimension comes from the record sizes: GRU units and GRU input
 * widths are multiples of 64 up to 512, every other layer has 1 to 512 rows,
 * dec_final 80, the conv kernel size is 1 to 8.  A side whose records are
 * missing, mis-sized, of unsupported dimensions, in an fp32 blob, or carry
 * int8 weights in which a maddubs pair can saturate is refused: its calls
 * return -1 with the reason in lpcnet_mi355x_last_error, and synthesis and
 * every other call behave as ever.
 * Each stream's encoder state (the three GRU states and the conv memory) and
 * decoder state (the three GRU states) live in buffers of their own,
 * allocated zeroed by the first of these calls; lpcnet_batch_reset does not
 * touch them (lpcnet_reset knows nothing of DRED), lpcnet_batch_rdovae_reset
 * zeroes them (DRED_rdovae_init_encoder / _decoder).
 * Out of scope: the statistical model (dred_*_q8 / q10 / q15) and the entropy
 * coding of latents, an fp32 RDO-VAE, emulating maddubs saturation, and
 * writing decoded frames into the concealment machine's FEC queue on the
 * device (reorder decode_all's output and use lpcnet_batch_conceal_fec_add). */
/* dims[24]: encoder {L, S, T, conv kernel size, the eight stack widths,
 * gdense1} at [0..12], decoder {L, S, T, the eight stack widths} at [13..23];
 * zeros for a side without usable records; -1 (last_error: both reasons) only
 * when neither side is usable.  Host only. */
LPCNET_EXPORT int lpcnet_mi355x_rdovae_dims(const unsigned char *data, int len, int dims[24]);
LPCNET_EXPORT int lpcnet_batch_rdovae_info(const LPCNetBatch *b, int dims[24]);
/* dred_rdovae_encode_dframe for every stream s with active[s] != 0 (NULL:
 * all): in [B][40] -> latents [B][L], initial_state [B][S]; rows of inactive
 * streams are not written, their state does not move. */
LPCNET_EXPORT int lpcnet_batch_rdovae_encode(LPCNetBatch *b, const float *in, float *latents, float *initial_state,
                                             const unsigned char *active);
/* the same on device buffers, queued on the batch's stream (lpcnet_batch_sync
 * waits): d_features [2][B][row], row 20 or 36 -- what
 * lpcnet_batch_compute_features_device writes for two frames; the first 20
 * values of frame 0 and of frame 1 are the input */
LPCNET_EXPORT int lpcnet_batch_rdovae_encode_device(LPCNetBatch *b, const float *d_features, int row, float *d_latents,
                                                    float *d_state, const unsigned char *d_active);
/* dred_rdovae_dec_init_states: state [B][S] -> the streams' decoder state */
LPCNET_EXPORT int lpcnet_batch_rdovae_dec_init(LPCNetBatch *b, const float *state, const unsigned char *active);
LPCNET_EXPORT int lpcnet_batch_rdovae_dec_init_device(LPCNetBatch *b, const float *d_state, const unsigned char *d_active);
/* dred_rdovae_decode_qframe on the streams' decoder state: latents [B][L] ->
 * qframe [B][80], four frames in reverse order */
LPCNET_EXPORT int lpcnet_batch_rdovae_decode_qframe(LPCNetBatch *b, const float *latents, float *qframe, const unsigned char *active);
LPCNET_EXPORT int lpcnet_batch_rdovae_decode_qframe_device(LPCNetBatch *b, const float *d_latents, float *d_qframe,
                                                           const unsigned char *d_active);
/* DRED_rdovae_decode_all: state [B][S], latents [B][n][L] -> features
 * [B][4 n][20] in the reference's own order, on a temporary state -- the
 * streams' decoder state is neither read nor written.  n == 0: nothing, 0. */
LPCNET_EXPORT int lpcnet_batch_rdovae_decode_all(LPCNetBatch *b, const float *state, const float *latents, float *features, int n,
                                                 const unsigned char *active);
LPCNET_EXPORT int lpcnet_batch_rdovae_decode_all_device(LPCNetBatch *b, const float *d_state, const float *d_latents,
                                                        float *d_features, int n, const unsigned char *d_active);
/* which: 1 the encoder's state, 2 the decoder's, 3 both (the encoder's
 * first).  reset: stream -1 is every stream.  A snapshot is the GRU states
 * dense2 | dense4 | dense6 and, for the encoder, the conv memory
 * [(kernel size - 1)][T], the oldest input first. */
LPCNET_EXPORT int lpcnet_batch_rdovae_reset(LPCNetBatch *b, int stream, int which);
LPCNET_EXPORT int lpcnet_batch_rdovae_state_size(const LPCNetBatch *b, int which);
LPCNET_EXPORT int lpcnet_batch_rdovae_save_state(LPCNetBatch *b, int stream, int which, void *buf);
LPCNET_EXPORT int lpcnet_batch_rdovae_restore_state(LPCNetBatch *b, int stream, int which, const void *buf);

/* Last error string of this thread. */
LPCNET_EXPORT const char *lpcnet_mi355x_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
