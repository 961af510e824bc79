/*
 * lpcnet_engine.h -- internal declarations of the MI355X LPCNet engine.
 * Shared by the host engine (engine.cpp) and the HIP kernels (kernels.hip).
 */
#ifndef LPCNET_ENGINE_H
#define LPCNET_ENGINE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernel_choice.h" /* OVERLAP_MAX_STREAMS, CHUNK_MIN_FRAMES, MF2_MIN_STREAMS, mfw_groups */

namespace lpcnet_mi355x {

/* Default model dimensions (training_tf2/lpcnet.py:312-325; the reference
 * bakes them into the generated nnet_data.h). */
constexpr int NA = 384;        /* GRU_A units */
constexpr int NB = 16;         /* GRU_B units */
constexpr int COND = 128;      /* conditioning size */
constexpr int NF = 20;         /* NB_FEATURES */
constexpr int EP = 64;         /* pitch embedding */
constexpr int FIN = NF + EP;   /* lpcnet.c:44 FRAME_INPUT_SIZE */
constexpr int NLPC = 16;       /* LPC_ORDER */
constexpr int FRAME = 160;     /* samples per frame */
constexpr int NBANDS = 18;     /* freq.h:48 NB_BANDS (cepstral bands of the 1.6 kb/s decoder) */
constexpr int GA_ROWS = 3 * NA;
constexpr int GB_ROWS = 3 * NB;
/* Model constants the reference bakes into the generated nnet_data.h
 * (dump_lpcnet.py:423-446, from train_lpcnet.py --lookahead / --lpc-gamma /
 * --end2end); here load-time parameters of a model (ModelConst). */
constexpr int DEFAULT_FEATURES_DELAY = 2; /* dump_lpcnet.py:441 default lookahead */
constexpr int MAX_FEATURES_DELAY = 4;     /* train_lpcnet.py:273 trims (4 - lookahead) frames: lookahead <= 4 */
constexpr int SAMPLE_THREADS = 384; /* one thread per GRU_A unit */
constexpr int SAMPLE_WAVES = SAMPLE_THREADS / 64;
constexpr int STAMP_WAVES = 8;      /* stamps are [workgroup][STAMP_WAVES][16] */
constexpr int FRAME_STREAMS = 4;    /* streams per frame-network workgroup */
constexpr int FRAME_PREFETCH = 64;  /* zero input rows padding each frame-network weight matrix */
constexpr int REG_GB = 12;          /* GRU_B input slots per lane: block k = ks + 8*j, j < 12 */
/* Matrix-core kernel (mf_kernel.hip).
 * GRU_A (v_mfma_i32_4x4x4_16b_i8): per-lane register tables, one u32 word
 * per slot.  Lane l of GRU_A wave w = (row group l/4 of the wave's 64 units,
 * row l%4 of the group); word k of the table holds
 *   [0, 16)   z-gate weight rows, slot t  (4 int8 = one row of an 8x4 block)
 *   [16, 32)  r-gate weight rows
 *   [32, 64)  h-gate weight rows
 *   [64, 80)  column-block bytes of those 64 slots (4 per word)
 * Unused slots hold zero weights and column block 0.
 * GRU_B (v_mfma_i32_16x16x64_i8, sampler waves): dense int8 A tiles, lane l
 * = row 16g + l%16, bytes k = 64kt + 16(l/16) + 0..15: tiles [g*6 + kt]
 * (input, 3 gates x 6 K tiles) then [18 + g] (recurrent, K = 16 in lanes
 * 0..15), [MF_GB_TILES][64 lanes] uint4. */
constexpr int MF_ZMAX = 16;         /* z / r slots per lane */
constexpr int MF_HMAX = 32;         /* h slots per lane */
constexpr int MF_GA = 2 * MF_ZMAX + MF_HMAX;
constexpr int MF_LANE_U32 = MF_GA + MF_GA / 4; /* 80 */
/* mfw_kernel split form (mf_plan.cpp mfw_split_tables): two host waves after
 * the six R waves carry the pieces of block rows beyond the register caps */
constexpr int MFW_H_WAVES = 2;
constexpr int MFW_TAB_WAVES = 6 + MFW_H_WAVES; /* SAMPLE_WAVES R waves + the host waves */
constexpr int MFW_NOROW = 0x1FF;               /* frow entry: no part row */
constexpr int MFW_PART_ROWS = 128;             /* part rows per gate: 16 unit blocks x 8 */
constexpr int MF_GB_IN = 3 * 6;                 /* GRU_B input tiles (3 gates x 6 K tiles) */
constexpr int MF_GB_TILES = MF_GB_IN + 3;        /* + the 3 recurrent tiles */
constexpr int MF_XSTR = 416;        /* LDS bytes per stream of the quantized GRU_A state (stream-major):
                                       104 dwords = 8 banks (mod 32) apart, so the 4 streams of
                                       input quad c occupy banks c + {0, 8, 16, 24} (mod 32) */
constexpr int MF_THREADS = 512;     /* 6 GRU_A waves + 2 sampler waves */
/* fp32 latency kernel (fp_kernel.hip), one stream per workgroup.
 * GRU_A per-lane tables (lane l of wave w = unit 64w + l = row l%8 of row
 * block 8w + l/8 of each gate; slot t = the t-th 8x4 block of that row block,
 * as the float4 of this row's 4 columns):
 *   fp_zr [wave][2][FP_ZF][64] float4: slot t as packed (z, r) pairs,
 *         [z.x r.x z.y r.y] then [z.z r.z z.w r.w] (registers)
 *   fp_h  [wave][FP_HF][64] float4: h slots (streamed from L2 every sample)
 *   fp_off [wave][FP_OFF_WORDS][64] u32: column-quad bytes, 4 per word, of
 *         the z, r and h slots
 * Unused slots hold -0.0 weights and column quad NA/4, which the kernel
 * keeps at +0.0: fma(-0, +0, y) = y for every y, NaN and -0 included.
 * fp_gb [NA/4][GB_ROWS] float4: dense GRU_B input weights (column quad,
 * row), copied to LDS. */
constexpr int FP_ZF = 16;           /* z / r slots per lane */
constexpr int FP_HF = 32;           /* h slots per lane */
constexpr int FP_OFF_WORDS = (2 * FP_ZF + FP_HF) / 4;
constexpr int FP_THREADS = 448;     /* 6 GRU_A waves + 1 sampler wave */

/* Per-stream synthesis state in device memory (lpcnet_private.h:28-48). */
struct alignas(16) StreamState {
  float gru_a_state[NA];
  float gru_a_cond[GA_ROWS];
  float gru_b_cond[GB_ROWS];
  float gru_b_state[NB];
  float last_sig[NLPC];
  float lpc[NLPC];
  float old_lpc[MAX_FEATURES_DELAY][NLPC]; /* lpc_from_cepstrum ring, first `delay` rows used */
  float conv1_mem[FIN * 2];
  float conv2_mem[COND * 2];
  float deemph_mem;
  int last_exc;
  int frame_count;
  uint32_t rng[4];
  /* LPCNetDecState::vq_mem (lpcnet_private.h:50-53): the previous packet's
   * last cepstrum, read by decode_packet (lpcnet_dec.c:81-156); zero after
   * a reset (lpcnet_decoder_init memsets the decoder state) */
  float vq_mem[NBANDS];
  int pad[3];
};

/* The device rcpps table holds t + kRcpBias (device_math.h rcp_x86_fix),
 * indexed by the top RCP_TABLE_BITS mantissa bits of the Pade denominator:
 * 12, so one table format holds both the Intel build host's rcpps (a
 * function of the top 11 bits: each entry twice) and the AMD EPYC GPU-box
 * host's (a function of the top 12 bits, profiles/r03/box_rcpps.json). */
constexpr uint32_t kRcpBias = 127u << 23;
constexpr int RCP_TABLE_BITS = 12;
constexpr int RCP_ENTRIES = 1 << RCP_TABLE_BITS;

/* Fixed sections of the sample kernel's LDS image (byte offsets). */
constexpr int IMG_RCP = 0;                       /* RCP_ENTRIES u32 rcpps table */
constexpr int IMG_ULAW = IMG_RCP + RCP_ENTRIES * 4; /* 256 f32 ulaw2lin */
constexpr int IMG_LOGIT = IMG_ULAW + 256 * 4;    /* 256 f32 sampling logit table */
constexpr int IMG_FCW = IMG_LOGIT + 256 * 4;     /* dual_fc weights [256][2][16] f32 */
constexpr int IMG_FCB = IMG_FCW + 256 * 32 * 4;  /* dual_fc bias [2][256] */
constexpr int IMG_FCF = IMG_FCB + 512 * 4;       /* dual_fc factor [2][256] */
constexpr int IMG_VAR = IMG_FCF + 512 * 4;       /* start of the variable sections */

/* What one frame step hands from the frame kernel to the sample kernel,
 * double-buffered by the overlapped multi-frame path (frame kernel f+1 runs
 * beside sample kernel f): the conditioning vectors, the LPC of this frame
 * and frame_count after this frame's update. */
constexpr int ZC_FEAT_MAX = 4096; /* host-I/O ticks up to this size read the features from mapped host memory */
constexpr int TICK_SPIN_MS = 20;  /* a host-I/O tick polls its end this long before a blocking wait */
constexpr int TICK_POLL_PAUSE = 0; /* x86 pause instructions between two polls */

struct alignas(16) FrameCond {
  float gru_a_cond[GA_ROWS];
  float gru_b_cond[GB_ROWS];
  float lpc[NLPC];
  int frame_count;
  int pad[3];
};

/* FEATURES_DELAY (lookahead frames: the LPC ring depth, the conv2 clear and
 * the silent first frames, lpcnet.c:101,109-112,239), LPC_GAMMA
 * (lpc_weighting, lpcnet.c:116-118) and END2END (LPC from the frame
 * network's rc outputs, lpcnet.c:56-80,107-108) of a model. */
struct ModelConst {
  float lpc_gamma;
  int delay;
  int end2end;
};

struct FrameArgs {
  StreamState *st;
  ModelConst mc;
  int nstreams;
  const float *features; /* [B][NF] for this frame */
  const float *lpc_new;  /* [B][NLPC] lpc_from_cepstrum(features) (lpc_kernel) */
  const float *conv1_w, *conv1_b, *conv2_w, *conv2_b;
  const float *dense1_w, *dense1_b, *dense2_w, *dense2_b;
  const float *gadf_w, *gadf_b, *gbdf_w, *gbdf_b;
  const float *proj_w, *proj_b; /* gadf | gbdf as one [COND][GA_ROWS + GB_ROWS] matrix, bias */
  const float *embed_pitch;
  const uint32_t *rcp; /* RCP_ENTRIES-entry table in global memory */
  unsigned long long *stamps; /* optional diagnostics [grid][16] s_memtime per phase */
  /* chunk_kernel only: features = [nframes][B][NF], lpc_new = [nframes][B][NLPC],
   * outputs of frame f into cond[f * B .. f * B + B) */
  int nframes;
  FrameCond *cond;
  /* frame_kernel: 1 = run_frame_network into the caller's locals, as
   * run_frame_network_flush does (lpcnet.c:134-144): conv memories, LPC ring
   * and frame_count advance, the state's conditioning and lpc stay */
  int keep_cond;
  int rcp_hw; /* chunk_kernel: hardware-reciprocal tanh allowed (see SampleArgs::rcp_hw) */
  /* chunk_kernel: the same five weight matrices re-tiled for 16-byte
   * per-lane loads (ck_tile_weights): [row tile][k quad][64 lanes] float4,
   * lane l = (g, r) = (l / 16, l % 16), element j of quad q = W[4 (4q + j) +
   * g][16 rt + r] (0 past K), CK_WPAD zero quads after each row tile's last */
  const float4 *ck_conv1, *ck_conv2, *ck_dense1, *ck_dense2, *ck_proj;
  /* conv1 .. dense2 are stored CK_SLICES_MAX times: copy k at + k ck_rep[i]
   * float4s (projection slice k of the one-frame kernel reads copy k) */
  int ck_rep[4];
  /* one-frame chunk_kernel, deferred LPC (FEATURES_DELAY >= 1): the frame's
   * LPC comes from the ring only, the ring is advanced later by lpc_kernel
   * (launch_lpc with a ring), and the frame's features are copied to
   * lpc_feat ([B][NF], device memory) for it when non-null */
  int lpc_defer;
  float *lpc_feat;
  /* one-frame chunk_kernel with its projection split over row slices
   * (launch_chunk picks the slice count): per 16-stream group an arrival
   * counter (zeroed, [groups]); a timed-out wait sets STATUS_SLICE_TIMEOUT
   * in *status (the batch's status word) */
  int *ck_sync;
  int *status;
};
constexpr int CK_SLICES_MAX = 4; /* projection slices of the one-frame chunk kernel */
constexpr int CK_WPAD = 8; /* chunk_kernel: k quads in flight per wave (zero padding of each row tile) */

struct SampleArgs {
  StreamState *st;
  int delay;             /* FEATURES_DELAY: a stream synthesises once frame_count > delay (lpcnet.c:239) */
  const FrameCond *cond; /* optional [B]: read the frame's outputs here instead of st */
  int nstreams;
  int N;                 /* samples to produce (<= FRAME) */
  int nframes;           /* mf_kernel: frames per launch (0 = 1).  Frame f reads cond + f B and
                            writes pcm + f B N; needs cond, preload 0, no trace, and every
                            stream active in all or none of the frames (the host splits a run
                            at the `delay` transition, STATUS_ACTIVITY otherwise) */
  short *pcm;            /* [B][N] */
  int preload;           /* samples 0..preload-1 are teacher-forced from pcm (lpcnet.c:256-259) */
  const float *emb_sig, *emb_pred, *emb_exc; /* [256][GA_ROWS] */
  const float *ga_par;   /* [6][NA]: recurrent bias z,r,h then diag z,r,h */
  const int *ga_wsum;    /* [3][NA]: 128*rowsum(int8 w) (non-saturating int8 path) */
  const float *gb_par;   /* [2][GB_ROWS]: input bias, recurrent bias */
  const int *gb_wsum;    /* [2][GB_ROWS] */
  const uint4 *image;    /* LDS image */
  int image_bytes;
  int image_lds_bytes;   /* lockstep kernel: bytes of the image copied to LDS (image_bytes, or IMG_VAR
                            when the weight sections stay in global memory) */
  int ga_K[SAMPLE_WAVES][3];   /* blocks per lane for wave w, gate g (padded) */
  int ga_woff[SAMPLE_WAVES][3];/* weight chunk offset (u32 units in image / float4 units in ga_wf) */
  int ga_coff[SAMPLE_WAVES][3];/* column-block index chunk offset (u16 units in image) */
  int gb_nb[GB_ROWS / 8];      /* blocks per GRU_B row block */
  int gb_woff[GB_ROWS / 8];    /* u32 units in image [k][8] / float4 [k][8][2] in gb_wf */
  int gb_coff[GB_ROWS / 8];    /* u16 units in image */
  int gb_rec_off;              /* byte offset of GRU_B recurrent int8 weights in image */
  /* quad int8 path (LDS image): per wave w / GRU_B row block, group of 4 slots gi:
   * weights [gi][64 lanes] uint4 at *_qoff (uint4 units), column blocks
   * [gi][8] u32 (4 x u8, one per lane octet) at *_coff (u32 units) */
  int ga_K4[SAMPLE_WAVES][3];
  int ga_qoff[SAMPLE_WAVES][3];
  int gb_qoff[GB_ROWS / 8];
  /* matrix-core kernel: GRU_A per-lane register tables [wave][MF_LANE_U32][64
   * lanes], 4-slot groups per wave (z/r padded to a common count, h); GRU_B
   * A tiles [MF_GB_TILES][64] */
  const uint32_t *mf;
  const int *mf_unit;                /* [SAMPLE_WAVES * 64]: GRU_A unit of each lane */
  float mf_zr_bound;                 /* |GRU_A z/r conditioning| below this (and finite) for a workgroup's
                                        streams: the elementwise step's range selects are dead (mf_kernel);
                                        negative: never */
  float mf_h_bound;                  /* the same for the h gate's conditioning (tanh range: the gate's
                                        input stays below device_math.h's kTanhFinBound) */
  int fc_fin;                        /* every dual-FC node sum |bias| + 2 sum|w| is finite and below
                                        kTanhFinBound (2^30): with GRU_B states within [-2, 2] (int8 models keep them
                                        there; checked per launch) the walk's tanh takes the
                                        select-free form */
  const float *mf_emb[3];            /* sig/pred/exc tables with columns in lane order:
                                        [256][3][SAMPLE_WAVES * 64], column p = unit mf_unit[p] */
  int mf_nzr[SAMPLE_WAVES];          /* own 4-slot groups per GRU_A wave: z and r */
  int mf_nh[SAMPLE_WAVES];           /* h */
  /* split models (rows longer than the own cap, mf_plan.cpp mf_plan): hosted
   * 4-slot groups after the own ones, the row each lane's hosted partial
   * sums belong to [3 gates][SAMPLE_WAVES * 64] (NA: none) */
  int mf_split;
  int mf_nfzr[SAMPLE_WAVES];
  int mf_nfh[SAMPLE_WAVES];
  const int *mf_frow;
  /* mfw_kernel's split form: [MFW_TAB_WAVES][MF_LANE_U32][64] tables (R
   * waves own rows to the full caps, host waves the pieces), group counts,
   * frow [3][SAMPLE_THREADS + 64 MFW_H_WAVES] (see mfw_split_tables) */
  int mfw_split;
  const uint32_t *mfw_tab;
  const int *mfw_frow;
  const int *mfw_unit;      /* [SAMPLE_THREADS]: the split form's own unit of each E / R lane */
  const float *mfw_emb[3];  /* embedding tables in the split form's lane order (as mf_emb) */
  int mfw_nzr[MFW_TAB_WAVES];
  int mfw_nh[MFW_TAB_WAVES];
  const uint4 *mf_gb;
  const float4 *fp_zr, *fp_h, *fp_gb; /* fp_kernel tables (see FP_ZF) */
  const uint32_t *fp_off;
  int fp_nzr[SAMPLE_WAVES];    /* slots of the z/r chains per GRU_A wave */
  int fp_nh[SAMPLE_WAVES];     /* slots of the h chains */
  /* fp_kernel long form (block rows beyond FP_ZF / FP_HF): every slot
   * streamed, [wave][slot][64 lanes]: z/r packed pairs (2 float4), h float4,
   * offsets (z quad | r quad << 8 for fpl_kz slots, then h quads) */
  int fp_long;
  int fpl_kz, fpl_kh;
  const float4 *fpl_zr, *fpl_h;
  const uint32_t *fpl_off;
  const float4 *ga_wf;   /* fp32 variant: GRU_A blocks [chunk][k][64] float4 */
  const float4 *gb_wf;   /* fp32 variant: GRU_B blocks [rb][k][8 rows][2] float4 (in c) */
  const float *gb_recf;  /* fp32 variant: GRU_B recurrent [NB][GB_ROWS] */
  unsigned long long *stamps; /* optional diagnostics [grid][STAMP_WAVES][16] s_memtime sums */
  float *trace_logits;   /* optional [B][N][8] */
  int *trace_exc;        /* optional [B][N] */
  int rcp_hw;            /* 1: the latency chains may use the hardware-reciprocal rcpps (equal to the
                            default Intel table only); 0: every activation through the LDS table
                            (lpcnet_batch_set_rcp_table with another host's table) */
  int *status;           /* device view of the batch's pinned status word: a
                            kernel that aborts sets bits (STATUS_*), the host
                            checks after every sync */
  int spin_limit;        /* polls before an LDS flag wait aborts (FLAG_SPIN_LIMIT_DEFAULT) */
};

constexpr int FLAG_SPIN_LIMIT_DEFAULT = 1 << 20; /* lpcnet_batch_set_spin_limit */
constexpr int FLAG_SPIN_LIMIT_MAX = 1 << 30;     /* larger requests are clamped (int poll counters) */
/* Status bits a sample kernel reports to the host (SampleArgs::status). */
constexpr int STATUS_FLAG_TIMEOUT = 1; /* an LDS flag wait exceeded spin_limit: output invalid */
constexpr int STATUS_ACTIVITY = 2;     /* a multi-frame launch saw a stream become active mid-launch */
constexpr int STATUS_SLICE_TIMEOUT = 4; /* a sliced chunk_kernel's writer waited too long for its siblings */

/* The frame step's outputs as a sample kernel reads them: the FrameCond
 * copy when the launch has one, else the stream state. */
#if defined(__HIP__) || defined(__HIPCC__)
/* the same with the frame's conditioning array given (multi-frame launches) */
__device__ __forceinline__ int frame_count_of(const SampleArgs &A, const FrameCond *cf, int sid)
{
  return cf ? cf[sid].frame_count : A.st[sid].frame_count;
}
__device__ __forceinline__ const float *gru_a_cond_of(const FrameCond *cf, const SampleArgs &A, int sid)
{
  return cf ? cf[sid].gru_a_cond : A.st[sid].gru_a_cond;
}
__device__ __forceinline__ const float *gru_b_cond_of(const FrameCond *cf, const SampleArgs &A, int sid)
{
  return cf ? cf[sid].gru_b_cond : A.st[sid].gru_b_cond;
}
__device__ __forceinline__ const float *lpc_of(const FrameCond *cf, const SampleArgs &A, int sid)
{
  return cf ? cf[sid].lpc : A.st[sid].lpc;
}
__device__ __forceinline__ int frame_count_of(const SampleArgs &A, int sid)
{
  return A.cond ? A.cond[sid].frame_count : A.st[sid].frame_count;
}
__device__ __forceinline__ const float *gru_a_cond_of(const SampleArgs &A, int sid)
{
  return A.cond ? A.cond[sid].gru_a_cond : A.st[sid].gru_a_cond;
}
__device__ __forceinline__ const float *gru_b_cond_of(const SampleArgs &A, int sid)
{
  return A.cond ? A.cond[sid].gru_b_cond : A.st[sid].gru_b_cond;
}
__device__ __forceinline__ const float *lpc_of(const SampleArgs &A, int sid)
{
  return A.cond ? A.cond[sid].lpc : A.st[sid].lpc;
}
#endif

/* Host helpers shared by the launchers (engine.cpp), thread-safe and keyed
 * by the current HIP device: raise a kernel's dynamic-LDS limit to `bytes`
 * once per (kernel, device); the CU count of the current device. */
int ensure_dyn_lds(const void *kernel, int bytes);
int current_device_cus();

/* Kernel launchers (kernels.hip).  variant: 0 int8, 1 fp32. sat: int8 pairs
 * may saturate. lds_bytes from sample_lds_bytes(). */
int sample_lds_bytes(int S, int variant, int image_bytes);
int launch_frame(const FrameArgs &a, void *stream);
constexpr int FK_ONE_STREAM_MAX = 256; /* frame kernel: one stream per workgroup up to this batch */
int frame_groups(int nstreams);        /* frame kernel workgroups (stamp rows) for a batch */
/* copy the frame step's outputs of every stream into cond[B] */
int launch_cond_copy(const StreamState *st, FrameCond *cond, int nstreams, void *stream);
/* dst[dmap ? dmap[k] : k] = src[smap ? smap[k] : k], k < n (device index maps) */
int launch_state_copy(StreamState *dst, const StreamState *src, const int *dmap, const int *smap, int n, void *stream);
int launch_sample(const SampleArgs &a, int S, int variant, int sat, int reg, int lds_bytes, void *stream);

/* Frame network of up to LPC_CHUNK frames in one launch (chunk_kernel.hip):
 * f32 matrix cores, 64 (stream, frame) columns per workgroup. */
int launch_chunk(const FrameArgs &a, void *stream);
/* Matrix-core kernel (non-saturating int8 models within the MF_* limits):
 * GRU_A recurrent product on v_mfma_i32_4x4x4_16b_i8 in the GRU_A waves,
 * GRU_B products on v_mfma_i32_16x16x64_i8 in the sampler waves, two
 * workgroup barriers per sample. */
int mf_lds_bytes(int S, int split);
int launch_mf(const SampleArgs &a, int S, int lds_bytes, void *stream);
/* Large batches: two groups of S streams per workgroup, half a sample
 * apart (mf2_kernel.hip); no preload / trace / stamps. */
int mf2_lds_bytes(int split);
int launch_mf2(const SampleArgs &a, void *stream);
/* wide-batch kernel (mfw_kernel.hip): 2 or 3 four-stream groups per
 * 896-thread workgroup with dedicated gather/elementwise, recurrent and
 * sampler waves (split models: two groups, 1,024 threads with two host
 * waves); int8 models with the default (Intel) rcpps, no preload / trace /
 * stamps (-1 otherwise) */
/* group count and selection: kernel_choice.h (mfw_groups, MFW_G3_PHASE) */
int mfw_lds_bytes(int groups, int split = 0);
int launch_mfw(const SampleArgs &a, int groups, void *stream);
/* fp32 latency kernel: one stream per workgroup, LDS flags instead of
 * workgroup barriers (fp32 models within the FP_* limits, dense GRU_B). */
int fp_lds_bytes();
int launch_fp(const SampleArgs &a, void *stream);

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
  int rcp_hw;                  /* as SampleArgs::rcp_hw */
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
 * LPCNetPLCState (lpcnet_private.h:78-106) the causal modes carry, and the
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
};
enum { CONCEAL_DC_REMOVE = 0, CONCEAL_DC_RESTORE = 1, CONCEAL_DC_CONCEAL = 2 };
/* the DC filter on io [B][FRAME] (lpcnet_plc.c:195-204, 283-287, 330-335): one lane per stream */
int launch_conceal_dc(const ConcealData &d, const int *idx, int n, short *io, int mode, void *stream);
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
/* work order [n][NF] / [n][N] from the streams' rows: w_feat (null: none) from
 * features (defer_row < 0) or the deferred buffer's row; w_pcm (null: none)
 * from st->pcm (src_buf) or the io row, at src_off */
int launch_conceal_gather(const ConcealData &d, const int *idx, int n, float *w_feat, int defer_row, short *w_pcm, const short *io,
                          int src_buf, int src_off, int N, void *stream);
/* w_pcm [n][N] to the io rows at dst_off, or to tmp (io null) */
int launch_conceal_scatter(const ConcealData &d, const int *idx, int n, const short *w_pcm, short *io, int dst_off, int N,
                           void *stream);
/* lpcnet_reset_signal (lpcnet.c:226-233) on st[idx[k]]; ulaw0 = lin2ulaw(0.f) */
int launch_conceal_reset_signal(StreamState *st, const int *idx, int n, int ulaw0, void *stream);
/* lpcnet_plc_fec_add's RNN_MOVE (:121) and RNN_COPY (:126) on one stream */
int launch_conceal_fec_compact(const ConcealData &d, int s, int from, int rows, void *stream);
int launch_conceal_fec_store(const ConcealData &d, int s, int pos, const float *features /* host, [NF] */, void *stream);

}  // namespace lpcnet_mi355x

#endif
