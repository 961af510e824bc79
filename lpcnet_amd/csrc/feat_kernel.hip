/*
 * feat_kernel.hip -- lpcnet_compute_single_frame_features for every stream of
 * a batch on the GPU: preemphasis, compute_frame_features and
 * process_single_frame (lpcnet_enc.c:872-880, 488-577, 814-870) with
 * pcount = 0, one wavefront per stream, FEAT_WG_STREAMS streams per workgroup,
 * __syncthreads between the stages.
 *
 * Restates, term for term and in the reference's operation order:
 *   preemphasis              lpcnet_enc.c:872-880  lane per sample (an FIR)
 *   frame_analysis           :488-496   window, forward Opus kiss FFT
 *                                       (lpc_stages.h), real input
 *   lpcn_compute_band_energy freq.c:131-154        lane per band, serial walk
 *   log10 + follower         lpcnet_enc.c:512-520  double log10 (device library)
 *   dct                      freq.c:218-228
 *   lpc_from_cepstrum        freq.c:310-320        lpc_stages.h, as lpc_kernel
 *   LPC residual             lpcnet_enc.c:525-537  lane per sample (an FIR)
 *   cross-correlation        :539-552   lane per lag; the double running
 *                                       energy on one lane per half-frame
 *   3x interpolation         :553-570
 *   Viterbi + backtrack      :824-866   lane per state, strict > everywhere
 * feat_kernel<true> is the same analysis for frame k of the 1.6 kb/s
 * encoder's superframe, without process_single_frame (enc_kernel.hip).
 * Must be compiled with -ffp-contract=off.
 */
#include <hip/hip_runtime.h>

#include "side_kernels.h"
#include "lpc_stages.h"

namespace lpcnet_mi355x {

namespace {

/* streams (waves) per workgroup: 4 measured fastest (2 / 4 / 8: 0.048 / 0.044 /
 * 0.050 ms at 1,024 streams, 0.520 / 0.467 / 0.498 at 32,768; profiles/r10) */
#ifndef FEAT_WG_STREAMS
#define FEAT_WG_STREAMS 4
#endif
constexpr int FS = FEAT_WG_STREAMS;
constexpr int WIN = LPC_WIN;
constexpr int HALF = FRAME / 2;      /* TRAINING_OFFSET, and the half-frame of the pitch search */
constexpr int EXC = PITCH_MAX + FRAME; /* exc_buf entries the single-frame path touches */
constexpr int NST = PITCH_STATES;
/* per-stream scratch floats */
constexpr int SM_EX = 0;    /* [NBANDS] band energies, then their logs */
constexpr int SM_CEPS = 18; /* [NBANDS] */
constexpr int SM_LPC = 36;  /* [NLPC] */
constexpr int SM_IP = 52;   /* ener0 of half-frame 0, 1; the 79-term start of ener1 of 0, 1 */
constexpr int SM_N = 64;
/* float view of a wave's FFT buffer once the spectrum is consumed */
constexpr int YF_ENER = 0;   /* [2][PITCH_MAX] `ener` of every lag; later [PITCH_MAX] pitch_max_path[0] */
constexpr int YF_PREV = 512; /* [2][NST] bytes: pitch_prev */
static_assert(YF_PREV * 4 + 2 * NST <= WIN * 8, "pitch_prev fits the FFT buffer");

}  // namespace

/* SUPER false: the single-frame extractor.  SUPER true: frame A.k of a
 * superframe (lpcnet_encode / lpcnet_compute_features, lpcnet_enc.c:882-909):
 * preemphasis and compute_frame_features with pcount = A.k, no
 * process_single_frame; the frame's two xc rows (before the sub-harmonic
 * check, which process_superframe runs) and frame_weights go to A.xc_out /
 * A.fw_out, its cepstrum to A.features and its LPC to A.lpc_out, all scratch
 * of the call that enc_kernel.hip consumes; the Viterbi state stays untouched. */
template <bool SUPER>
__global__ __launch_bounds__(64 * FS) void feat_kernel(FeatArgs A)
{
  __shared__ C2 ybuf[FS][WIN];
  __shared__ C2 tw[WIN];
  __shared__ float dct[NBANDS * NBANDS];
  __shared__ LpcSlot slot[WIN];
  __shared__ float hwin[FRAME], frac[FRAME];
  __shared__ int bstart[NBANDS];
  __shared__ float Eb[FS][NBANDS + 2];
  __shared__ float acb[FS][LPC_ORDER1];
  __shared__ float excb[FS][EXC];
  __shared__ float xcb[FS][2][PITCH_MAX];
  __shared__ float smb[FS][SM_N];
  __shared__ int liveb[FS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int sid = blockIdx.x * FS + w;
  const bool live = sid < A.nstreams && (!A.active || A.active[sid]); /* wave-uniform */
  if (lane == 0) liveb[w] = live;
  const LpcTables *T = A.lpc_tab;
  stage_fft_dct<true>(T, tw, dct, slot);
  stage_bands<true>(A.tab, frac, bstart, hwin);
  const double sq = T->sqrt_2_18;
  const float cmp = lane < NBANDS ? T->comp[lane] : 0.f, scale = T->scale;
  FeatState *S = A.state + (live ? sid : 0);
  C2 *y = ybuf[w];
  float *yf = (float *)ybuf[w];
  float *exc = excb[w], *sm = smb[w];
  float(*xc)[PITCH_MAX] = xcb[w];
  /* aligned_in behind its 16 predecessors: al[NLPC + i] = aligned_in[i],
   * al[NLPC - 1 - j] = pitch_mem[j]; in xc's second row, which the
   * cross-correlation writes two barriers after the residual last read it */
  float *al = xcb[w][1];
  float *out = A.features + (size_t)(live ? sid : 0) * A.stride;
  __syncthreads(); /* the tables stand (the window below reads hwin) */

  /* preemphasis (lpcnet_enc.c:872-880: y = x + mem, mem = -coef x), the
   * window over analysis_mem | in (:488-493, freq.c:322-328) into the FFT's
   * digit-reversed scaled slots (kiss_fft.c:570-578), aligned_in (:510, 526)
   * and the carried exc_buf (:525) */
  float in_r[3] = {0.f, 0.f, 0.f};
  float x_last = 0.f;
  if (live) {
#pragma unroll
    for (int t = 0; t < 3; t++) {
      const int i = lane + 64 * t;
      if (i < FRAME) {
        const size_t o = (size_t)sid * FRAME + i;
        const float x = A.pcm ? (float)A.pcm[o] : A.pcm_f[o];
        float mem = S->mem_preemph;
        if (i > 0) mem = -PREEMPH_COEF * (A.pcm ? (float)A.pcm[o - 1] : A.pcm_f[o - 1]);
        const float v = x + mem;
        in_r[t] = v;
        if (i == FRAME - 1) x_last = x;
        const float am = S->analysis_mem[i];
        y[fft_slot(i)] = C2{scale * (am * hwin[i]), scale * 0.f};
        y[fft_slot(FRAME + i)] = C2{scale * (v * hwin[FRAME - 1 - i]), scale * 0.f};
        if (i >= HALF) al[NLPC + i - HALF] = am;
        else al[NLPC + HALF + i] = v;
      }
    }
    if (lane < NLPC) al[NLPC - 1 - lane] = S->pitch_mem[lane];
    for (int k = lane; k < PITCH_MAX; k += 64) exc[k] = S->exc[k];
  }
  __syncthreads();
  fft320_stages(live, lane, y, tw);

  /* lpcn_compute_band_energy (freq.c:131-154), lpc_stages.h's walk */
  if (live && lane < NBANDS) {
    const float sum = band_energy_walk(lane, y, frac, bstart, [](float p) { return p; });
    /* log10(1e-2+Ex[i]) in double, rounded to float (lpcnet_enc.c:515) */
    sm[SM_EX + lane] = (float)log10(1e-2 + (double)sum);
  }
  __syncthreads();

  /* the logMax / follow recursion (lpcnet_enc.c:512-520), repeated by every
   * band's lane, then that lane's dct output (freq.c:218-228) */
  if (live && lane < NBANDS) {
    float logMax = -2, follow = -2, acc = 0;
#pragma unroll
    for (int i = 0; i < NBANDS; i++) {
      float ly = sm[SM_EX + i];
      ly = MAX16(logMax - 8, MAX16(follow - 2.5f, ly));
      logMax = MAX16(logMax, ly);
      follow = MAX16(follow - 2.5f, ly);
      acc += ly * dct[i * NBANDS + lane];
    }
    float c = (float)((double)acc * sq);
    if (lane == 0) c -= 4;
    sm[SM_CEPS + lane] = c;
    out[lane] = c;
  }
  __syncthreads();

  /* lpc_from_cepstrum (lpcnet_enc.c:523) */
  float ceps[NBANDS];
#pragma unroll
  for (int j = 0; j < NBANDS; j++) ceps[j] = sm[SM_CEPS + j];
  lpc_autocorr_stages(live, lane, ceps, y, Eb[w], acb[w], LpcLds{tw, dct, slot, sq, cmp, scale});
  /* as lpc_kernel: wave 0 runs every stream's recursion, a lane each */
  if (w == 0 && lane < FS && liveb[lane]) {
    float lpc[NLPC];
    levinson16(acb[lane], lpc);
#pragma unroll
    for (int i = 0; i < NLPC; i++) smb[lane][SM_LPC + i] = lpc[i];
  }
  __syncthreads();

  /* LPC residual (lpcnet_enc.c:527-537): pitch_mem[j] = aligned_in[i-1-j] */
  float s_last = 0.f;
  if (live) {
    if constexpr (SUPER) {
      if (lane < NLPC) A.lpc_out[(size_t)sid * NLPC + lane] = sm[SM_LPC + lane];
    } else {
      if (A.row == NTF && lane < NLPC) out[NF + lane] = sm[SM_LPC + lane];
    }
#pragma unroll
    for (int t = 0; t < 3; t++) {
      const int i = lane + 64 * t;
      if (i < FRAME) {
        float sum = al[NLPC + i];
#pragma unroll
        for (int j = 0; j < NLPC; j++) sum += sm[SM_LPC + j] * al[NLPC + i - 1 - j];
        yf[i] = sum;
        if (i == FRAME - 1) s_last = sum;
      }
    }
  }
  __syncthreads();
  if (live)
#pragma unroll
    for (int t = 0; t < 3; t++) {
      const int i = lane + 64 * t;
      if (i < FRAME) exc[PITCH_MAX + i] = yf[i] + .7f * (i ? yf[i - 1] : S->pitch_filt);
    }
  __syncthreads();

  /* celt_pitch_xcorr on both half-frames (lpcnet_enc.c:542; pitch.c:44-83:
   * every lag's sum in j order), and the inner products of :543-544 */
  if (live) {
#pragma unroll
    for (int sub = 0; sub < 2; sub++) {
      const float *x = exc + PITCH_MAX + sub * HALF, *yv = exc + sub * HALF;
      float sum[4] = {0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < HALF; j++) {
        const float xj = x[j];
#pragma unroll
        for (int t = 0; t < 4; t++) sum[t] += xj * yv[lane + 64 * t + j];
      }
#pragma unroll
      for (int t = 0; t < 4; t++) xc[sub][lane + 64 * t] = sum[t];
    }
    if (lane < 4) {
      const int sub = lane & 1;
      const float *x = (lane & 2) ? exc + sub * HALF : exc + PITCH_MAX + sub * HALF;
      const int n = (lane & 2) ? HALF - 1 : HALF;
      float xy = 0;
      for (int j = 0; j < n; j++) xy += x[j] * x[j];
      sm[SM_IP + lane] = xy;
    }
  }
  __syncthreads();
  /* ener of every lag (lpcnet_enc.c:547-552): the double running energy, one
   * lane per half-frame; 1 + ener0 is a float sum, + ener1 a double one */
  if (live && lane < 2) {
    const int off = lane * HALF;
    const float e0 = 1 + sm[SM_IP + lane];
    double ener1 = sm[SM_IP + 2 + lane];
    for (int i = 0; i < PITCH_MAX; i++) {
      const float a = exc[i + off + HALF - 1];
      ener1 += a * a;
      yf[YF_ENER + lane * PITCH_MAX + i] = (float)(e0 + ener1);
      const float c = exc[i + off];
      ener1 -= c * c;
    }
  }
  __syncthreads();
  if (live)
#pragma unroll
    for (int sub = 0; sub < 2; sub++)
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const int i = lane + 64 * t;
        xc[sub][i] = 2 * xc[sub][i] / yf[YF_ENER + sub * PITCH_MAX + i];
      }
  __syncthreads();

  /* 3x interpolation (lpcnet_enc.c:553-570): only j = 6's interpolated[i]
   * survives, and it reads the un-updated row */
  float nv[2][4];
  if (live) {
    const float interp[7] = {0.026184f, -0.098339f, 0.369938f, 0.837891f, -0.184969f, 0.070242f, -0.020947f};
#pragma unroll
    for (int sub = 0; sub < 2; sub++)
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const int i = lane + 64 * t;
        nv[sub][t] = xc[sub][i];
        if (i >= 4 && i < PITCH_MAX - 4) {
          float val1 = 0, val2 = 0;
#pragma unroll
          for (int j = 0; j < 7; j++) {
            val1 += xc[sub][i - 3 + j] * interp[j];
            val2 += xc[sub][i + 3 - j] * interp[j];
          }
          nv[sub][t] = MAX16(xc[sub][i], MAX16(val1, val2));
        }
      }
    if constexpr (SUPER) {
      /* rows 2 + 2 k + sub of xc and frame_weight (lpcnet_enc.c:545-570) */
#pragma unroll
      for (int sub = 0; sub < 2; sub++) {
        float *row = A.xc_out + ((size_t)sid * 8 + 2 * A.k + sub) * PITCH_MAX;
#pragma unroll
        for (int t = 0; t < 4; t++) row[lane + 64 * t] = nv[sub][t];
      }
      if (lane < 2) A.fw_out[(size_t)sid * 8 + 2 * A.k + lane] = sm[SM_IP + lane];
      /* what crosses frames, but for the Viterbi state */
#pragma unroll
      for (int t = 0; t < 3; t++)
        if (lane + 64 * t < FRAME) S->analysis_mem[lane + 64 * t] = in_r[t];
      if (lane < NLPC) S->pitch_mem[NLPC - 1 - lane] = in_r[1];
      for (int k = lane; k < PITCH_MAX; k += 64) S->exc[k] = exc[FRAME + k];
      if (lane == (FRAME - 1) % 64) {
        S->mem_preemph = -PREEMPH_COEF * x_last;
        S->pitch_filt = s_last;
      }
    } else {
      /* pitch_max_path[0] into the FFT buffer (the ener values are consumed) */
      for (int k = lane; k < PITCH_MAX; k += 64) yf[YF_ENER + k] = S->pitch_max_path[k];
    }
  }
  if constexpr (SUPER) return; /* the whole workgroup: no barrier is left waiting */
  __syncthreads();
  if (live)
#pragma unroll
    for (int sub = 0; sub < 2; sub++)
#pragma unroll
      for (int t = 0; t < 4; t++) xc[sub][lane + 64 * t] = nv[sub][t];
  __syncthreads();
  /* the sub-harmonic check (lpcnet_enc.c:827-830): every read before any write */
  if (live)
#pragma unroll
    for (int sub = 0; sub < 2; sub++) subharmonic_row(xc[sub], lane, nv[sub]);
  __syncthreads();
  if (live)
#pragma unroll
    for (int sub = 0; sub < 2; sub++)
#pragma unroll
      for (int t = 0; t < 3; t++) xc[sub][lane + 64 * t] = nv[sub][t];
  __syncthreads();

  /* process_single_frame (lpcnet_enc.c:814-870) */
  float fw[2];
  {
    float fws = 1e-15f;
    fws += sm[SM_IP + 0];
    fws += sm[SM_IP + 1];
    fw[0] = sm[SM_IP + 0] * (2.f / fws);
    fw[1] = sm[SM_IP + 1] * (2.f / fws);
  }
  float *pmp = yf + YF_ENER;
  unsigned char *pprev = (unsigned char *)(yf + YF_PREV);
  float max_all = live ? S->pitch_max_path_all : 0.f;
  int best_i = live ? S->best_i : 0;
#pragma unroll
  for (int sub = 0; sub < 2; sub++) viterbi_step(live, lane, pmp, xc[sub], fw[sub], pprev + sub * NST, max_all, best_i);

  if (live) {
    /* backward pass (lpcnet_enc.c:856-866) */
    if (lane == 0) {
      int bi = best_i, best[2];
      float frame_corr = 0;
      for (int sub = 1; sub >= 0; sub--) {
        best[sub] = PITCH_MAX - bi;
        frame_corr += fw[sub] * xc[sub][bi];
        bi = pprev[sub * NST + bi];
      }
      frame_corr /= 2;
      int p = best[0] + best[1];
      p = p < 510 ? p : 510;
      p = p > 66 ? p : 66;
      out[NBANDS] = .01f * (p - 200);
      out[NBANDS + 1] = frame_corr - .5f;
      S->pitch_max_path_all = max_all;
      S->best_i = best_i;
    }
    /* what crosses frames */
#pragma unroll
    for (int t = 0; t < 3; t++)
      if (lane + 64 * t < FRAME) S->analysis_mem[lane + 64 * t] = in_r[t];
    if (lane < NLPC) S->pitch_mem[NLPC - 1 - lane] = in_r[1]; /* aligned_in[159-j] = in[79-j] */
    for (int k = lane; k < PITCH_MAX; k += 64) S->exc[k] = exc[FRAME + k];
    for (int k = lane; k < NST; k += 64) S->pitch_max_path[k] = pmp[k];
    if (lane == (FRAME - 1) % 64) { /* the lane of the frame's last sample */
      S->mem_preemph = -PREEMPH_COEF * x_last;
      S->pitch_filt = s_last;
    }
  }
}

int launch_feat(const FeatArgs &a, void *stream)
{
  if (a.nstreams < 1 || (a.row != NF && a.row != NTF) || a.stride < a.row || (!a.pcm && !a.pcm_f) || !a.features || !a.state) return -1;
  const int grid = (a.nstreams + FS - 1) / FS;
  hipLaunchKernelGGL(feat_kernel<false>, dim3(grid), dim3(64 * FS), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_feat_super(const FeatArgs &a, void *stream)
{
  if (a.nstreams < 1 || a.row != NF || a.stride != NF || !a.pcm || !a.features || !a.state || !a.xc_out || !a.fw_out || !a.lpc_out || a.k < 0 || a.k > 3)
    return -1;
  const int grid = (a.nstreams + FS - 1) / FS;
  hipLaunchKernelGGL(feat_kernel<true>, dim3(grid), dim3(64 * FS), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace lpcnet_mi355x
