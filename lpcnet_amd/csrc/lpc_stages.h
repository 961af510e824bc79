/*
 * lpc_stages.h -- the device stages lpc_kernel.hip, feat_kernel.hip,
 * burg_kernel.hip and enc_kernel.hip share, one wavefront per stream:
 *   the constant tables' staging into LDS, the FFT's input permutation
 *   the Opus 320-point kiss FFT (factors 4,4,4,5; kiss_fft.c:101-305, 518-586)
 *   lpc_from_cepstrum (freq.c:310-320)
 *   the band-energy walk of lpcn_compute_band_energy and its inverse form
 *   the pitch search's sub-harmonic check and Viterbi forward step
 * The stages that end in __syncthreads() say so: all threads of the
 * workgroup must call them, live stream or not.
 * Must be compiled with -ffp-contract=off.
 */
#ifndef LPCNET_LPC_STAGES_H
#define LPCNET_LPC_STAGES_H

#include <hip/hip_runtime.h>

#include "side_kernels.h"
#include "pow10_dd.h"

namespace lpcnet_mi355x {

namespace {

#define MAX16(a, b) ((a) > (b) ? (a) : (b)) /* arch.h:73 */
#define MIN16(a, b) ((a) < (b) ? (a) : (b)) /* arch.h:72 */

constexpr float PREEMPH_COEF = 0.85f; /* freq.h:34 PREEMPHASIS */

struct alignas(8) C2 {
  float r, i;
};

/* The constant tables into a workgroup's LDS, every thread of it a share; the
 * caller's next __syncthreads() makes them stand.  Which tables a kernel has
 * is a template argument, not a null pointer: a run-time test of an LDS
 * pointer stays in the loop and keeps it from unrolling (feat_kernel<true>
 * +1.2 % at 32,768 streams, profiles/r18).
 * The FFT's twiddles, with SLOTS the band and fraction of every FFT slot
 * (interp_band_gain) in the same loop -- a loop each costs lpc_kernel 14 VGPRs
 * and two waves per SIMD -- and the dct matrix: */
template <bool SLOTS>
__device__ __forceinline__ void stage_fft_dct(const LpcTables *T, C2 *tw, float *dct, LpcSlot *slot)
{
  for (int k = threadIdx.x; k < LPC_WIN; k += blockDim.x) {
    tw[k] = C2{T->twr[k], T->twi[k]};
    if constexpr (SLOTS) slot[k] = T->slot[k];
  }
  for (int k = threadIdx.x; k < NBANDS * NBANDS; k += blockDim.x) dct[k] = T->dct[k];
}

/* the band-energy walk's fractions and band starts, with WINDOW the analysis
 * window's rising half */
template <bool WINDOW>
__device__ __forceinline__ void stage_bands(const FeatTables *F, float *frac, int *bstart, float *hwin)
{
  for (int k = threadIdx.x; k < FRAME; k += blockDim.x) {
    if constexpr (WINDOW) hwin[k] = F->half_window[k];
    frac[k] = F->frac[k];
  }
  if (threadIdx.x < NBANDS) bstart[threadIdx.x] = F->band_start[threadIdx.x];
}

/* kiss_fft's input permutation for factors (4,4,4,5): sample n = d0 + 5 d1 +
 * 20 d2 + 80 d3 feeds FFT slot 64 d0 + 16 d1 + 4 d2 + d3 (build_lpc_tables) */
__device__ __forceinline__ int fft_slot(int n)
{
  const int d3 = n / 80, r = n % 80, d2 = r / 20, r2 = r % 20, d1 = r2 / 5, d0 = r2 % 5;
  return 64 * d0 + 16 * d1 + 4 * d2 + d3;
}

__device__ __forceinline__ C2 cmul(C2 a, C2 b) { return C2{a.r * b.r - a.i * b.i, a.r * b.i + a.i * b.r}; }
__device__ __forceinline__ C2 cadd(C2 a, C2 b) { return C2{a.r + b.r, a.i + b.i}; }
__device__ __forceinline__ C2 csub(C2 a, C2 b) { return C2{a.r - b.r, a.i - b.i}; }

/* radix-4 butterfly j of a group at p (kiss_fft_bfly4, kiss_fft.c:164-214,
 * m > 1 form; m == 1 has no twiddles) */
__device__ __forceinline__ void bfly4(C2 *p, int j, int m, int tstride, const C2 *tw)
{
  if (m == 1) {
    C2 f0 = p[0], f1 = p[1], f2 = p[2], f3 = p[3];
    const C2 s0 = csub(f0, f2);
    f0 = cadd(f0, f2);
    C2 s1 = cadd(f1, f3);
    f2 = csub(f0, s1);
    f0 = cadd(f0, s1);
    s1 = csub(f1, f3);
    p[0] = f0;
    p[2] = f2;
    p[1] = C2{s0.r + s1.i, s0.i - s1.r};
    p[3] = C2{s0.r - s1.i, s0.i + s1.r};
    return;
  }
  C2 *q = p + j;
  const C2 a = cmul(q[m], tw[j * tstride]);
  const C2 b = cmul(q[2 * m], tw[2 * j * tstride]);
  const C2 c = cmul(q[3 * m], tw[3 * j * tstride]);
  C2 q0 = q[0];
  const C2 d = csub(q0, b);
  q0 = cadd(q0, b);
  const C2 e = cadd(a, c), h = csub(a, c);
  q[2 * m] = csub(q0, e);
  q[0] = cadd(q0, e);
  q[m] = C2{d.r + h.i, d.i - h.r};
  q[3 * m] = C2{d.r - h.i, d.i + h.r};
}

/* radix-5 butterfly u of the last stage, m = 64 (kiss_fft_bfly5, kiss_fft.c:255-305) */
__device__ __forceinline__ void bfly5(C2 *f, int u, const C2 *tw)
{
  const int m = 64;
  const C2 ya = tw[m], yb = tw[2 * m];
  C2 *q0 = f + u, *q1 = q0 + m, *q2 = q0 + 2 * m, *q3 = q0 + 3 * m, *q4 = q0 + 4 * m;
  const C2 s0 = *q0;
  const C2 s1 = cmul(*q1, tw[u]), s2 = cmul(*q2, tw[2 * u]), s3 = cmul(*q3, tw[3 * u]), s4 = cmul(*q4, tw[4 * u]);
  const C2 s7 = cadd(s1, s4), s10 = csub(s1, s4), s8 = cadd(s2, s3), s9 = csub(s2, s3);
  C2 r0;
  r0.r = s0.r + (s7.r + s8.r);
  r0.i = s0.i + (s7.i + s8.i);
  const C2 s5{s0.r + ((s7.r * ya.r) + (s8.r * yb.r)), s0.i + ((s7.i * ya.r) + (s8.i * yb.r))};
  const C2 s6{(s10.i * ya.i) + (s9.i * yb.i), -((s10.r * ya.i) + (s9.r * yb.i))};
  const C2 s11{s0.r + ((s7.r * yb.r) + (s8.r * ya.r)), s0.i + ((s7.i * yb.r) + (s8.i * ya.r))};
  const C2 s12{(s9.i * ya.i) - (s10.i * yb.i), (s10.r * yb.i) - (s9.r * ya.i)};
  *q0 = r0;
  *q1 = csub(s5, s6);
  *q4 = cadd(s5, s6);
  *q2 = cadd(s11, s12);
  *q3 = csub(s11, s12);
}

/* opus_fft_impl on a wave's 320 digit-reversed, scaled slots y (written and
 * synchronised by the caller), one lane per butterfly.  Radix-4 stages:
 * (m, groups, span, twiddle stride) = (1, 80, 4, 80), (4, 20, 16, 20),
 * (16, 5, 64, 5), then the radix-5 stage with m = 64. */
__device__ __forceinline__ void fft320_stages(bool live, int lane, C2 *y, const C2 *tw)
{
  if (live)
    for (int t = lane; t < 80; t += 64) bfly4(y + 4 * t, 0, 1, 80, tw);
  __syncthreads();
  if (live)
    for (int t = lane; t < 80; t += 64) bfly4(y + 16 * (t >> 2), t & 3, 4, 20, tw);
  __syncthreads();
  if (live)
    for (int t = lane; t < 80; t += 64) bfly4(y + 64 * (t >> 4), t & 15, 16, 5, tw);
  __syncthreads();
  if (live) bfly5(y, lane, tw);
  __syncthreads();
}

/* the constant tables of the stages below, staged in LDS by the caller */
struct LpcLds {
  const C2 *tw;        /* [LPC_WIN] */
  const float *dct;    /* [NBANDS * NBANDS] */
  const LpcSlot *slot; /* [LPC_WIN] */
  double sq;           /* LpcTables::sqrt_2_18 */
  float cmp;           /* LpcTables::comp[lane] (lanes below NBANDS) */
  float scale;         /* LpcTables::scale */
};

/* lpc_from_cepstrum up to the windowed autocorrelation (freq.c:230-240,
 * 316-318, 202-216, 256-296): lanes below NBANDS hold the stream's cepstrum
 * in ceps[]; y [LPC_WIN], E [NBANDS + 2] and ac [LPC_ORDER1] are the wave's
 * LDS.  ac is complete after the last barrier. */
__device__ __forceinline__ void lpc_autocorr_stages(bool live, int lane, const float (&ceps)[NBANDS], C2 *y, float *E,
                                                    float *ac, const LpcLds &L)
{
  /* idct + band powers (freq.c:230-240, 316-318) */
  if (live && lane < NBANDS) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < NBANDS; j++) {
      const float t = j == 0 ? ceps[0] + 4 : ceps[j];
      acc += t * L.dct[lane * NBANDS + j];
    }
    const float ex = (float)((double)acc * L.sq);
    E[lane] = (float)(pow10_dd((double)ex) * (double)L.cmp);
  }
  __syncthreads();

  /* scaled Hermitian spectrum in digit-reversed order (freq.c:202-216, 256-268;
   * kiss_fft_stride's input permutation and 1/nfft scaling): FFT slot i holds
   * bin perm[i]; bins above 160 are the conjugates (imaginary -0.f) */
  if (live)
    for (int i = lane; i < LPC_WIN; i += 64) {
      const LpcSlot sl = L.slot[i];
      float g = 0.f;
      if (sl.band < NBANDS - 1) g = (1 - sl.frac) * E[sl.band] + sl.frac * E[sl.band + 1];
      y[i] = C2{L.scale * g, L.scale * (sl.conj ? -0.f : 0.f)};
    }
  __syncthreads();
  fft320_stages(live, lane, y, L.tw);

  /* autocorrelation, noise floor and lag window (freq.c:268-296) */
  if (live && lane < LPC_ORDER1) {
    float a = LPC_WIN * y[lane == 0 ? 0 : LPC_WIN - lane].r;
    if (lane == 0) a += a * 1e-4 + 320 / 12 / 38.;
    else a *= (1 - 6e-5 * lane * lane);
    ac[lane] = a;
  }
  __syncthreads();
}

/* Levinson-Durbin, float build of lpcn_lpc (freq.c:86-127), on one lane;
 * fully unrolled, so lpc[] and ac[] stay in registers (a dynamic index into
 * a register array costs a select chain per access) */
__device__ __forceinline__ void levinson16(const float *acs, float (&lpc)[LPC_ORDER1 - 1])
{
  float ac[LPC_ORDER1];
#pragma unroll
  for (int i = 0; i < LPC_ORDER1; i++) ac[i] = acs[i];
  float err = ac[0];
#pragma unroll
  for (int i = 0; i < LPC_ORDER1 - 1; i++) lpc[i] = 0;
  if (ac[0] != 0) {
#pragma unroll
    for (int i = 0; i < LPC_ORDER1 - 1; i++) {
      float rr = 0;
#pragma unroll
      for (int j = 0; j < i; j++) rr += lpc[j] * ac[i - j];
      rr += ac[i + 1];
      const float r = -rr / err;
      lpc[i] = r;
#pragma unroll
      for (int j = 0; j < (i + 1) >> 1; j++) {
        const float a = lpc[j], b = lpc[i - 1 - j];
        lpc[j] = a + r * b;
        lpc[i - 1 - j] = b + r * a;
      }
      err = err - (r * r) * err;
      if (err < .001f * ac[0]) break;
    }
  }
}

/* The walk of lpcn_compute_band_energy (freq.c:131-154) and
 * compute_band_energy_inverse (freq.c:60-84) for one band on one lane: sum
 * takes segment band-1's frac terms, then segment band's (1-frac) terms, each
 * in bin order; the end bands count twice.  term(|y|^2 as the reference sums
 * it) is what a bin contributes. */
template <class Term>
__device__ __forceinline__ float band_energy_walk(int band, const C2 *y, const float *frac, const int *bstart, Term term)
{
  float sum = 0;
  if (band > 0)
    for (int k = bstart[band - 1]; k < bstart[band]; k++) {
      float tmp = y[k].r * y[k].r;
      tmp += y[k].i * y[k].i;
      sum += frac[k] * term(tmp);
    }
  if (band < NBANDS - 1)
    for (int k = bstart[band]; k < bstart[band + 1]; k++) {
      float tmp = y[k].r * y[k].r;
      tmp += y[k].i * y[k].i;
      sum += (1 - frac[k]) * term(tmp);
    }
  if (band == 0 || band == NBANDS - 1) sum *= 2;
  return sum;
}

/* The sub-harmonic check of one xc row r (lpcnet_enc.c:607-610, 827-830), a
 * lane's entries lane + 64 t, t < 3, into nv.  It reads entries above i only
 * ((PITCH_MAX+i-1)/2 > i for i < 192), which the reference's serial loop has
 * not scaled yet: every read before any write, so the caller stores nv to the
 * row behind a __syncthreads(). */
__device__ __forceinline__ void subharmonic_row(const float *r, int lane, float *nv)
{
#pragma unroll
  for (int t = 0; t < 3; t++) {
    const int i = lane + 64 * t;
    const float xc_half = MAX16(MAX16(r[(PITCH_MAX + i) / 2], r[(PITCH_MAX + i + 2) / 2]), r[(PITCH_MAX + i - 1) / 2]);
    nv[t] = r[i];
    if (r[i] < xc_half * 1.1f) nv[t] = r[i] * .8f;
  }
}

/* One forward step of the pitch Viterbi search over one xc row with frame
 * weight fw (lpcnet_enc.c:604-635, 831-855), lane per state, strict >
 * everywhere: pmp [PITCH_STATES] is the wave's pitch_max_path, pprev
 * [PITCH_STATES] takes this row's pitch_prev, max_all / best_i carry
 * pitch_max_path_all and its index from row to row.  Two __syncthreads(). */
__device__ __forceinline__ void viterbi_step(bool live, int lane, float *pmp, const float *xc, float fw, unsigned char *pprev,
                                             float &max_all, int &best_i)
{
  constexpr int NST = PITCH_STATES;
  float pv[4] = {0.f, 0.f, 0.f, 0.f};
  float cur = -1e15f;
  int cur_i = 0;
  if (live) {
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int i = lane + 64 * t;
      if (i < NST) {
        float max_prev = max_all - 6.f;
        int pp = best_i;
#pragma unroll
        for (int j = -4; j <= 4; j++)
          if (j >= -i && i + j < NST) {
            const int aj = j < 0 ? -j : j;
            const float v = pmp[i + j] - .02f * aj * aj;
            if (v > max_prev) {
              max_prev = v;
              pp = i + j;
            }
          }
        pprev[i] = (unsigned char)pp;
        pv[t] = max_prev + fw * xc[i];
        if (pv[t] > cur) {
          cur = pv[t];
          cur_i = i;
        }
      }
    }
    /* the first index of the maximum, as the serial strict > keeps it */
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      const float ov = __shfl_xor(cur, m, 64);
      const int oi = __shfl_xor(cur_i, m, 64);
      if (ov > cur || (ov == cur && oi < cur_i)) {
        cur = ov;
        cur_i = oi;
      }
    }
  }
  __syncthreads();
  if (live) {
    /* renormalise; RNN_COPY's entries beyond NST are never written: they keep their zeros */
#pragma unroll
    for (int t = 0; t < 4; t++)
      if (lane + 64 * t < NST) pmp[lane + 64 * t] = pv[t] - cur;
    max_all = cur;
    best_i = cur_i;
  }
  __syncthreads();
}

}  // namespace

}  // namespace lpcnet_mi355x

#endif
