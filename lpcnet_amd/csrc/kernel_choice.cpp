/*
 * kernel_choice.cpp -- the sample-kernel and frame-path rules
 * (kernel_choice.h).  Host-only, system compiler, -ffp-contract=off as every
 * translation unit.
 */
#include "kernel_choice.h"

#include <stdlib.h>
#include <string.h>

extern char **environ;

namespace lpcnet_mi355x {

/* One pass over the environment instead of a getenv per switch: the live
 * one-frame tick reads them on every call.  The first entry of a name
 * counts, as for getenv. */
ChoiceEnv choice_env_from_env()
{
  static const char *const names[8] = {"LPCNET_MF2",           "LPCNET_MFW",        "LPCNET_MFW_G",     "LPCNET_NO_CHUNK",
                                       "LPCNET_NO_MULTIFRAME", "LPCNET_NO_OVERLAP", "LPCNET_LPC_EAGER", "LPCNET_NO_DIRECT_PCM"};
  const char *v[8] = {};
  for (char **p = environ; p && *p; p++) {
    if (strncmp(*p, "LPCNET_", 7)) continue;
    for (int k = 0; k < 8; k++) {
      const size_t n = strlen(names[k]);
      if (!v[k] && !strncmp(*p, names[k], n) && (*p)[n] == '=') v[k] = *p + n + 1;
    }
  }
  ChoiceEnv e;
  if (v[0]) e.mf2 = atoi(v[0]) != 0;
  if (v[1]) e.mfw = atoi(v[1]) != 0;
  if (v[2]) e.mfw_g = atoi(v[2]) == 2 ? 2 : 3;
  e.no_chunk = v[3] != nullptr;
  e.no_multiframe = v[4] != nullptr;
  e.no_overlap = v[5] != nullptr;
  e.lpc_eager = v[6] && atoi(v[6]) != 0;
  e.no_direct_pcm = v[7] != nullptr;
  return e;
}

int mfw_groups(int B, int cus)
{
  if (cus < 1 || B <= 4 * cus) return 0;
  const double c2 = (double)((B + 8 * cus - 1) / (8 * cus)) * 2;
  const double c3 = (double)((B + 12 * cus - 1) / (12 * cus)) * 3 * MFW_G3_PHASE;
  return c3 < c2 ? 3 : 2;
}

bool plans_wide(int B, int kernel_mode, bool rcp_custom, int cus, const ChoiceEnv &env)
{
  if ((kernel_mode != 0 && kernel_mode != 4) || rcp_custom) return false;
  if (env.mf2 == 0) return false;
  if (env.mfw >= 0) return env.mfw != 0;
  return mfw_groups(B, cus) > 0;
}

SamplePlan plan_sample_kernels(const ModelCaps &caps, const LdsSizes &lds, int B, int cus, int kernel_mode, bool rcp_custom,
                               const ChoiceEnv &env)
{
  SamplePlan p;
  p.cus = cus;
  int mode = kernel_mode;
  if (mode == 0) mode = caps.fp_ok ? 5 : (caps.mf_ok ? 4 : 1);
  /* a custom rcpps table (another host's, same-box parity): the fast
   * kernels run their table-only forms (the hardware-reciprocal shortcut is
   * proven for the Intel table only) */
  p.rcp_hw = rcp_custom ? 0 : 1;
  if (mode == 5 && caps.fp_ok && lds.fp <= 160 * 1024) {
    p.base = SampleKernel::FP;
    p.streams_per_workgroup = 1;
    p.lds_bytes = lds.fp;
    p.quad_path = 5;
    return p;
  }
  if (mode == 4 && caps.mf_ok && lds.mf <= 160 * 1024) {
    p.base = SampleKernel::MF;
    p.mfma_ops_per_group_sample = caps.mf_ga_ops + caps.mf_gb_ops;
    p.streams_per_workgroup = caps.S;
    p.lds_bytes = lds.mf;
    p.quad_path = 4;
    /* two staggered 4-stream groups per workgroup from MF2_MIN_STREAMS on
     * (LPCNET_MF2=0 off, =1 at any batch size); above one mf_kernel<4>
     * round, mfw_kernel (two or three groups with dedicated roles) where the
     * model allows it (LPCNET_MFW=0/1 off / on wherever mf2 runs,
     * LPCNET_MFW_G=2/3 forces the group count) */
    const int gauto = mfw_groups(B, cus);
    /* split models: the wide kernel's own split form where its tables exist
     * (mfw_split_tables), two groups only (LDS) */
    const bool mfw_ok = (!caps.mf_split || caps.mfw_split) && p.rcp_hw;
    const bool wantw = env.mfw >= 0 ? env.mfw != 0 : gauto > 0;
    p.mfw_forced = env.mfw > 0;
    const bool want2 = env.mf2 >= 0 ? env.mf2 != 0 : B >= MF2_MIN_STREAMS || (wantw && mfw_ok);
    if (want2 && lds.mf2 <= 160 * 1024) {
      p.mf2 = true;
      p.mfma_ops_per_group_sample = 2 * (caps.mf_ga_ops + caps.mf_gb_ops);
      p.streams_per_workgroup = 8;
      p.lds_bytes = lds.mf2;
      p.quad_path = 6;
      p.mfw_g = caps.mf_split ? 2 : env.mfw_g ? env.mfw_g : (gauto ? gauto : 2);
      if (wantw && mfw_ok && lds.mfw[p.mfw_g - 2] <= 160 * 1024) {
        p.mfw = true;
        p.mfma_ops_per_group_sample = p.mfw_g * (caps.mf_ga_ops + caps.mf_gb_ops);
        p.streams_per_workgroup = 4 * p.mfw_g;
        p.lds_bytes = lds.mfw[p.mfw_g - 2];
        p.quad_path = 7;
      }
    }
    return p;
  }
  p.streams_per_workgroup = caps.S;
  p.lds_bytes = caps.lds_bytes;
  p.quad_path = caps.reg ? 1 : 0;
  return p;
}

SampleKernel kernel_for_launch(const SamplePlan &plan, int nB, bool preload, bool trace, bool stamps)
{
  if (plan.base != SampleKernel::MF) return plan.base;
  const bool plain = !preload && !trace && !stamps;
  const bool wide = plan.mfw && (plan.mfw_forced || nB > 4 * plan.cus);
  if (wide && plain) return SampleKernel::MFW;
  if (plan.mf2 && (!plan.mfw || wide) && plain) return SampleKernel::MF2;
  return SampleKernel::MF;
}

FramePath frame_path(const SamplePlan &plan, int B, bool has_fstream, bool chunking, bool trace, bool stamps, int nframes,
                     int N, const ChoiceEnv &env)
{
  const bool mf = plan.base == SampleKernel::MF;
  /* the kernels reading the frame outputs through FrameCond */
  const bool cond = mf || plan.base == SampleKernel::FP;
  FramePath fp;
  /* multi-frame matrix-core sample launches (SampleLaunch::nframes): one
   * launch per chunk instead of one per frame (each costs a ~10 us dispatch
   * gap plus its prologue), behind the chunked frame network */
  fp.multi_frame = mf && chunking && !trace && N > 0 && nframes >= CHUNK_MIN_FRAMES && !env.no_multiframe;
  /* otherwise overlapped frame kernels: matrix-core and fp32 latency
   * kernels, when CUs are free */
  fp.overlapped = !fp.multi_frame && has_fstream && cond && nframes >= 2 && !stamps && !env.no_overlap;
  /* chunked frame network: batches too large for the overlapped path (the
   * sample kernels fill the GPU) */
  fp.chunked = fp.multi_frame ||
               (!fp.overlapped && chunking && cond && B > OVERLAP_MAX_STREAMS && !stamps && !env.no_chunk);
  return fp;
}

bool single_frame_chunked(const SamplePlan &plan, bool chunking, int nB, int N, int preload, bool trace, bool stamps,
                          const ChoiceEnv &env)
{
  return chunking && (plan.base == SampleKernel::MF || plan.base == SampleKernel::FP) && nB > OVERLAP_MAX_STREAMS && N > 0 &&
         preload == 0 && !stamps && !trace && !env.no_chunk;
}

bool lpc_deferred(int features_delay, int end2end, const ChoiceEnv &env)
{
  return !end2end && features_delay >= 1 && !env.lpc_eager;
}

bool pcm_store_coalesced(SampleKernel kernel, const ChoiceEnv &env)
{
  return !env.no_direct_pcm && (kernel == SampleKernel::FP || kernel == SampleKernel::MFW || kernel == SampleKernel::MF);
}

}  // namespace lpcnet_mi355x
