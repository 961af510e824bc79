/*
 * kernel_choice.h -- which sample kernel a batch and each of its launches
 * run, and which frame path a call takes.  Pure host functions: everything
 * they look at comes in through their arguments (the environment as a
 * ChoiceEnv), so the rules can be checked without a device
 * (lpcnet_mi355x_kernel_choice, tests/test_kernel_choice.py).  No HIP
 * include; engine.cpp (the plan) and synth_steps.cpp (the launches and
 * calls) are the callers.
 */
#ifndef LPCNET_KERNEL_CHOICE_H
#define LPCNET_KERNEL_CHOICE_H

namespace lpcnet_mi355x {

constexpr int OVERLAP_MAX_STREAMS = 128; /* batches up to this size get the overlapped multi-frame path (sample + frame workgroups fit the 256 CUs) */
constexpr int CHUNK_MIN_FRAMES = 4;      /* shorter runs use the per-frame kernel */
constexpr int MF2_MIN_STREAMS = 2048;    /* automatic choice of mf2_kernel from this batch size */
/* mfw_kernel runs in rounds of one workgroup per CU.  Per stream at whole
 * rounds (24,576 streams, same box, profiles/r05): two groups 7.07 ms per
 * frame, three 7.36 (per-phase time 1.04x), mf2_kernel 8.02 -- so two
 * groups replace mf2_kernel wherever both apply (same 8-stream rounds), and
 * three groups are taken where their 12-stream rounds save more than the 4 %
 * (3,072 streams: one round against two).  Above 4 streams per CU only:
 * below, mf_kernel's one-group latency wins. */
constexpr double MFW_G3_PHASE = 1.08; /* 1.04 before two groups took the LDS rcpps table (-3.4 %) */
/* 0 (batch within one mf_kernel<4> round), 2 or 3 */
int mfw_groups(int B, int cus);

/* The environment switches that steer the choice.  Read afresh wherever the
 * engine decides (each plan, each synthesis call), never cached: a process
 * may change them between two batches. */
struct ChoiceEnv {
  int mf2 = -1;   /* LPCNET_MF2: -1 unset, 0, 1 (any other number) */
  int mfw = -1;   /* LPCNET_MFW: the same */
  int mfw_g = 0;  /* LPCNET_MFW_G: 0 unset, 2, 3 (anything but 2) */
  bool no_chunk = false;      /* LPCNET_NO_CHUNK (set at all) */
  bool no_multiframe = false; /* LPCNET_NO_MULTIFRAME (set at all) */
  bool no_overlap = false;    /* LPCNET_NO_OVERLAP (set at all) */
  bool lpc_eager = false;     /* LPCNET_LPC_EAGER set and non-zero */
  bool no_direct_pcm = false; /* LPCNET_NO_DIRECT_PCM (set at all) */
};
ChoiceEnv choice_env_from_env();

/* what the choice takes from a HostModel */
struct ModelCaps {
  bool fp_ok = false;    /* fp32 model fits the fp_kernel tables */
  bool mf_ok = false;    /* model fits the matrix-core register tables */
  bool mf_split = false, mfw_split = false; /* split GRU_A plan; the wide kernel's split tables exist */
  bool reg = false;      /* lockstep kernel: quad layout */
  int S = 1;             /* lockstep / mf_kernel streams per workgroup */
  int lds_bytes = 0;     /* lockstep kernel */
  double mf_ga_ops = 0;  /* int8 matrix-core ops per workgroup per sample: the GRU_A recurrent pass */
  double mf_gb_ops = 0;  /* the GRU_B tiles of both sampler waves */
};

/* dynamic LDS of the kernels for this model (the .hip units' *_lds_bytes) */
struct LdsSizes {
  int fp = 0;            /* fp_lds_bytes() */
  int mf = 0;            /* mf_lds_bytes(S, mf_split) */
  int mf2 = 0;           /* mf2_lds_bytes(mf_split) */
  int mfw[2] = {0, 0};   /* mfw_lds_bytes(2 | 3, mf_split) */
};

enum class SampleKernel { LOCKSTEP = 0, MF = 1, MF2 = 2, MFW = 3, FP = 4 };

/* A batch's choice.  base: LOCKSTEP, MF or FP; on an MF batch, mf2 / mfw say
 * which kernel the launches without preload / trace / stamps get instead
 * (kernel_for_launch). */
struct SamplePlan {
  SampleKernel base = SampleKernel::LOCKSTEP;
  bool mf2 = false;        /* large batches: mf2_kernel (two staggered 4-stream groups per workgroup) */
  bool mfw = false;        /* wider batches: mfw_kernel (two or three 4-stream groups, dedicated gather /
                              recurrent / sampler waves; split models in its split form), models with the
                              default rcpps */
  bool mfw_forced = false; /* LPCNET_MFW=1: mfw_kernel for every launch, however narrow */
  int mfw_g = 3;           /* mfw_kernel's four-stream groups per workgroup (2 or 3) */
  int cus = 256;           /* compute units of the batch's device */
  int rcp_hw = 1;          /* SampleForm / FrameArgs::rcp_hw: 0 with a custom rcpps table */
  /* LPCNetModelInfo */
  int quad_path = 0, streams_per_workgroup = 1, lds_bytes = 0;
  double mfma_ops_per_group_sample = 0;
};

/* Sample-kernel choice (kernel_mode 0 = automatic):
 *   5  fp_kernel  -- fp32 models with a dense GRU_B within the FP_* limits
 *   4  mf_kernel  -- non-saturating int8 models within the MF_* limits
 *   1  sample_kernel (lockstep) -- every other model: saturating int8 models
 *      (int16 maddubs saturation emulated) and fp32 models with a sparse GRU_B.
 * A mode the model cannot run falls back to the lockstep kernel. */
SamplePlan plan_sample_kernels(const ModelCaps &caps, const LdsSizes &lds, int B, int cus, int kernel_mode, bool rcp_custom,
                               const ChoiceEnv &env);

/* whether plan_sample_kernels will run mfw_kernel on such a batch, the
 * model's own limits (split plan, LDS) aside: the plan class of its register
 * tables follows the same predicate */
bool plans_wide(int B, int kernel_mode, bool rcp_custom, int cus, const ChoiceEnv &env);

/* Per launch of nB streams.  A batch that runs mfw_kernel gives its launches
 * of at most one mf_kernel<4> round (nB <= 4 streams per CU: a drop-in
 * pool's work batch is sized for its widest launch, a partial step of a
 * batch) to mf_kernel, whose one-group sample is the shorter chain there;
 * mf2_kernel and mfw_kernel take no preload, trace or stamps. */
SampleKernel kernel_for_launch(const SamplePlan &plan, int nB, bool preload, bool trace, bool stamps);

/* lpcnet_batch_synthesize_frames: multi_frame = multi-frame matrix-core
 * sample launches behind the chunked frame network; otherwise overlapped =
 * frame kernel f+1 on the second queue beside sample kernel f (has_fstream:
 * the batch has that queue); chunked = the frame network of a chunk of frames
 * in one chunk_kernel launch. */
struct FramePath {
  bool multi_frame, overlapped, chunked;
};
FramePath frame_path(const SamplePlan &plan, int B, bool has_fstream, bool chunking, bool trace, bool stamps, int nframes,
                     int N, const ChoiceEnv &env);

/* one frame of a large batch in the chunked form (a live server's tick) */
bool single_frame_chunked(const SamplePlan &plan, bool chunking, int nB, int N, int preload, bool trace, bool stamps,
                          const ChoiceEnv &env);

/* Deferred LPC (one-frame ticks of models with FEATURES_DELAY >= 1): a
 * frame synthesises with the LPC of frame f - FEATURES_DELAY (lpcnet.c:
 * 110-118), already in the stream's ring, so lpc_from_cepstrum of this
 * frame's features is off the tick's critical path.  LPCNET_LPC_EAGER=1
 * keeps the LPC before the chunk kernel. */
bool lpc_deferred(int features_delay, int end2end, const ChoiceEnv &env);

/* sample kernels whose PCM write-out is wide (a frame's samples, or 16 of
 * them, per stream in consecutive lanes): mf_kernel at the end of the
 * launch, mfw_kernel every 16 samples, fp_kernel at the end.  mf2_kernel
 * stores every sample as it is drawn (2-byte stores: over PCIe, one
 * transaction each), so its PCM goes through device memory and one copy. */
bool pcm_store_coalesced(SampleKernel kernel, const ChoiceEnv &env);

}  // namespace lpcnet_mi355x

#endif
