/*
 * burg_kernel.hip -- burg_cepstral_analysis (freq.c:156-199) for every stream
 * of a batch on the GPU, in three launches on one stream.  No state across
 * frames, no weights.
 *   burg_acf_kernel   one wavefront per stream, BURG_WG_STREAMS streams per
 *                     workgroup: burg_in and the autocorrelations, one lane
 *                     per (half-frame, lag)
 *   burg_rec_kernel   one lane per (stream, half-frame), full wavefronts: the
 *                     order recursion.  It is a serial walk of some 5,000
 *                     instructions whose five double arrays want 250
 *                     registers; beside the other stages it would run on 2
 *                     of a wavefront's 64 lanes (burg_kernel)
 *   burg_ceps_kernel  one wavefront per stream, half-frame h on lanes
 *                     32 h .. 32 h + 31: transform, bands, log, dct
 * The stages hand over through per-call scratch (BurgArgs cbuf, xbuf, obuf),
 * column 2 s + h of 2 B, so a wavefront of the recursion reads and writes
 * consecutive addresses.
 *
 * Restates, term for term and in the reference's operation order:
 *   burg_in                  freq.c:169            lane per sample, float
 *   autocorrelation          burg.c:43-94, 117-125 lane per (half-frame, lag),
 *                                                  double, the 4-way grouping
 *   the order recursion      burg.c:128-217        one lane per (stream,
 *                                                  half-frame), double,
 *                                                  fully unrolled
 *   residual energy, A       burg.c:219-244        both forms
 *   gain, filter input       freq.c:171-174        float division; the pow
 *                                                  values are the host's
 *   forward_transform        freq.c:242-254        lpc_stages.h: fft_slot and
 *                                                  the scale, full butterflies
 *   compute_band_energy_inverse  freq.c:60-84      lane per band, serial walk
 *   scaling, log10, follower freq.c:177-183        double log10; the 2.5 of
 *                                                  the follower is a double
 *   dct, ceps[0] += -4       freq.c:184-185, 218-228
 *   .5*(c0+c1), (c0-c1)      freq.c:192-198
 * Inputs on which the reference build aborts (its asserts nrg_f > 0,
 * nrg_b > 0, |rc| < 1) are outside the contract.
 * Must be compiled with -ffp-contract=off.
 */
#include <hip/hip_runtime.h>

#include "side_kernels.h"
#include "lpc_stages.h"

namespace lpcnet_mi355x {

namespace {

#ifndef BURG_WG_STREAMS
#define BURG_WG_STREAMS 4 /* feat_kernel's FEAT_WG_STREAMS: a later fusion stays possible */
#endif
constexpr int BS = BURG_WG_STREAMS;
constexpr int WIN = LPC_WIN;
constexpr int HALF = FRAME / 2;
constexpr int L = BURG_LEN;           /* subfr_length of silk_burg_analysis */
constexpr int D = NLPC;               /* its order */
constexpr int NC = BURG_NC;           /* C0, lags 1..16, the energy of the first D samples */
constexpr float COND_FAC = 1e-5f;     /* burg.c:40 FIND_LPC_COND_FAC, a float literal */

/* silk_energy_FLP / silk_inner_product_FLP (burg.c:43-94): double products,
 * result += ((p0 + p1) + p2) + p3, then the remainder one by one */
__device__ __forceinline__ double inner_flp(const float *a, const float *b, int n)
{
  double result = 0.0;
  int i = 0;
  for (; i < n - 3; i += 4)
    result += a[i + 0] * (double)b[i + 0] + a[i + 1] * (double)b[i + 1] + a[i + 2] * (double)b[i + 2] + a[i + 3] * (double)b[i + 3];
  for (; i < n; i++) result += a[i] * (double)b[i];
  return result;
}

/* silk_burg_analysis(A, x, (float)1e-3, L, 1, D) after its autocorrelations
 * (burg.c:128-244) on one lane.  The recursion touches x[0..15] and
 * x[L-16..L-1] only: xa[j] = x[j], xb[j] = x[L - D + j]; C: C0,
 * C_first_row[0..15], silk_energy_FLP(x, D).  Every loop is unrolled, so the
 * five double arrays stay in registers.  Returns the residual energy. */
__device__ __forceinline__ float burg16(const float (&xa)[D], const float (&xb)[D], const double (&C)[NC], float (&A)[D])
{
  const float minInvGain = (float)1e-3; /* a float parameter (burg.c:101, freq.c:170) */
  double C0 = C[0];
  double Cf[D], Cl[D], CAf[D + 1], CAb[D + 1], Af[D];
#pragma unroll
  for (int k = 0; k < D; k++) {
    Cf[k] = Cl[k] = C[k + 1];
    Af[k] = 0.0;
    CAf[k + 1] = CAb[k + 1] = 0.0;
  }
  CAb[0] = CAf[0] = C0 + COND_FAC * C0 + 1e-9f;
  double invGain = 1.0f, rc, num, nrg_f, nrg_b, tmp1, tmp2, Atmp;
  bool reached = false;
#pragma unroll
  for (int n = 0; n < D; n++) {
    if (!reached) { /* the reference's break */
      const float xn = xa[n], xl = xb[D - 1 - n]; /* x[n], x[L-n-1] */
      tmp1 = xn;
      tmp2 = xl;
#pragma unroll
      for (int k = 0; k < n; k++) {
        /* float products, rounded to float before the double subtraction */
        Cf[k] -= xn * xa[n - k - 1];
        Cl[k] -= xl * xb[D - n + k];
        Atmp = Af[k];
        tmp1 += xa[n - k - 1] * Atmp;
        tmp2 += xb[D - n + k] * Atmp;
      }
#pragma unroll
      for (int k = 0; k <= n; k++) {
        CAf[k] -= tmp1 * xa[n - k];
        CAb[k] -= tmp2 * xb[D - n + k - 1];
      }
      tmp1 = Cf[n];
      tmp2 = Cl[n];
#pragma unroll
      for (int k = 0; k < n; k++) {
        Atmp = Af[k];
        tmp1 += Cl[n - k - 1] * Atmp;
        tmp2 += Cf[n - k - 1] * Atmp;
      }
      CAf[n + 1] = tmp1;
      CAb[n + 1] = tmp2;
      num = CAb[n + 1];
      nrg_b = CAb[0];
      nrg_f = CAf[0];
#pragma unroll
      for (int k = 0; k < n; k++) {
        Atmp = Af[k];
        num += CAb[n - k] * Atmp;
        nrg_b += CAb[k + 1] * Atmp;
        nrg_f += CAf[k + 1] * Atmp;
      }
      rc = -2.0 * num / (nrg_f + nrg_b);
      tmp1 = invGain * (1.0 - rc * rc);
      if (tmp1 <= minInvGain) {
        rc = sqrt(1.0 - minInvGain / invGain);
        if (num > 0) rc = -rc;
        invGain = minInvGain;
        reached = true;
      } else {
        invGain = tmp1;
      }
#pragma unroll
      for (int k = 0; k < (n + 1) >> 1; k++) {
        tmp1 = Af[k];
        tmp2 = Af[n - k - 1];
        Af[k] = tmp1 + rc * tmp2;
        Af[n - k - 1] = tmp2 + rc * tmp1;
      }
      Af[n] = rc; /* the coefficients beyond n keep their zeros (burg.c:203-209) */
      if (!reached) {
#pragma unroll
        for (int k = 0; k <= n + 1; k++) {
          tmp1 = CAf[k];
          CAf[k] += rc * CAb[n - k + 1];
          CAb[n - k + 1] += rc * tmp1;
        }
      }
    }
  }
  if (reached) {
    C0 -= C[D + 1];
    nrg_f = C0 * invGain;
#pragma unroll
    for (int k = 0; k < D; k++) A[k] = (float)(-Af[k]);
  } else {
    nrg_f = CAf[0];
    tmp1 = 1.0;
#pragma unroll
    for (int k = 0; k < D; k++) {
      Atmp = Af[k];
      nrg_f += CAf[k + 1] * Atmp;
      tmp1 += Atmp * Atmp;
      A[k] = (float)(-Atmp);
    }
    nrg_f -= COND_FAC * C0 * tmp1;
  }
  return (float)nrg_f;
}

}  // namespace

/* Stage 1, one wavefront per stream: burg_in, C0, C_first_row and the
 * silk_energy_FLP(x, D) of burg.c:226 into A.cbuf [NC][2 B], the 16 first and
 * 16 last samples of burg_in into A.xbuf [2 D][2 B]; column 2 s + h. */
__global__ __launch_bounds__(64 * BS) void burg_acf_kernel(BurgArgs A)
{
  __shared__ float pf[BS][FRAME];
  __shared__ float bi[BS][2][HALF];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int h = lane >> 5, l = lane & 31;
  const int sid = blockIdx.x * BS + w;
  const bool live = sid < A.nstreams && (!A.active || A.active[sid]); /* wave-uniform */
  const size_t n2 = 2 * (size_t)A.nstreams, col = 2 * (size_t)(live ? sid : 0) + h;
  /* the frame as floats */
  if (live)
    for (int i = lane; i < FRAME; i += 64) {
      const size_t o = (size_t)sid * FRAME + i;
      pf[w][i] = A.pcm ? (float)A.pcm[o] : A.pcm_f[o];
    }
  __syncthreads();
  /* burg_in (freq.c:169) of both half-frames */
  if (live)
    for (int i = lane; i < 2 * HALF; i += 64) {
      const int hh = i / HALF, j = i % HALF;
      if (j < L) bi[w][hh][j] = pf[w][hh * HALF + j + 1] - PREEMPH_COEF * pf[w][hh * HALF + j];
    }
  __syncthreads();
  if (live) {
    const float *x = bi[w][h];
    if (l < NC) A.cbuf[l * n2 + col] = l <= D ? inner_flp(x, x + l, L - l) : inner_flp(x, x, D);
    A.xbuf[l * n2 + col] = l < D ? x[l] : x[L - 2 * D + l];
  }
}

/* Stage 2, one lane per (stream, half-frame), full wavefronts: the order
 * recursion, the gain and the filter input (freq.c:170-174) into A.obuf
 * [D + 1][2 B]: x[1..16], then g.  Lanes of one wavefront read and write
 * consecutive columns. */
__global__ __launch_bounds__(64) void burg_rec_kernel(BurgArgs A)
{
  const size_t n2 = 2 * (size_t)A.nstreams, col = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (col >= n2 || (A.active && !A.active[col >> 1])) return;
  float xa[D], xb[D], a[D];
  double C[NC];
#pragma unroll
  for (int j = 0; j < D; j++) {
    xa[j] = A.xbuf[j * n2 + col];
    xb[j] = A.xbuf[(D + j) * n2 + col];
  }
#pragma unroll
  for (int k = 0; k < NC; k++) C[k] = A.cbuf[k * n2 + col];
  float g = burg16(xa, xb, C, a);
  g /= HALF - 2 * (D - 1);
#pragma unroll
  for (int i = 0; i < D; i++) A.obuf[i * n2 + col] = (float)(-a[i] * A.btab->pw[i]);
  A.obuf[D * n2 + col] = g;
}

/* Stage 3, one wavefront per stream, half-frame h on lanes 32 h .. 32 h + 31:
 * the transform of the filter input, the inverse band energies, log10, the
 * follower, the dct and the combination of the two half-frames. */
__global__ __launch_bounds__(64 * BS) void burg_ceps_kernel(BurgArgs A)
{
  __shared__ C2 ybuf[BS][2][WIN];
  __shared__ C2 tw[WIN];
  __shared__ float dct[NBANDS * NBANDS];
  __shared__ float frac[FRAME];
  __shared__ int bstart[NBANDS];
  __shared__ float xs[BS][2][D + 1];
  __shared__ float gs[BS][2];
  __shared__ float lyb[BS][2][NBANDS], cpb[BS][2][NBANDS];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int h = lane >> 5, l = lane & 31;
  const int sid = blockIdx.x * BS + w;
  const bool live = sid < A.nstreams && (!A.active || A.active[sid]); /* wave-uniform */
  const LpcTables *T = A.lpc_tab;
  stage_fft_dct<false>(T, tw, dct, nullptr);
  stage_bands<false>(A.tab, frac, bstart, nullptr);
  const double sq = T->sqrt_2_18;
  const float scale = T->scale;
  float *out = A.out + (size_t)(live ? sid : 0) * A.stride;
  if (live && l <= D) {
    const size_t n2 = 2 * (size_t)A.nstreams, col = 2 * (size_t)sid + h;
    if (l < D) xs[w][h][l + 1] = A.obuf[l * n2 + col];
    else {
      xs[w][h][0] = 1;
      gs[w][h] = A.obuf[D * n2 + col];
    }
  }
  __syncthreads();
  /* forward_transform (freq.c:242-254) of x, zero beyond its 17 taps, into
   * the FFT's digit-reversed scaled slots (kiss_fft.c:570-578) */
  if (live)
    for (int i = lane; i < 2 * WIN; i += 64) {
      const int hh = i / WIN, j = i % WIN;
      const float v = j <= D ? xs[w][hh][j] : 0.f;
      ybuf[w][hh][fft_slot(j)] = C2{scale * v, scale * 0.f};
    }
  __syncthreads();
  fft320_stages(live, lane, ybuf[w][0], tw);
  fft320_stages(live, lane, ybuf[w][1], tw);

  /* compute_band_energy_inverse (freq.c:60-84), lpc_stages.h's walk over
   * 1/(|y|^2 + 1e-9), a double sum and quotient rounded to float; the scaling
   * of :177 and the log10 of :179 */
  if (live && l < NBANDS) {
    float sum = band_energy_walk(l, ybuf[w][h], frac, bstart, [](float p) { return (float)(1.f / (p + 1e-9)); });
    sum = (float)(sum * (.45 * gs[w][h] * (1.f / ((float)WIN * WIN * WIN))));
    lyb[w][h][l] = (float)log10(1e-2 + sum);
  }
  __syncthreads();
  /* the logMax / follow recursion (freq.c:178-183; follow-2.5 is a double
   * difference here), repeated by every band's lane, then that lane's dct
   * output (freq.c:218-228) and ceps[0] += -4 */
  if (live && l < NBANDS) {
    float logMax = -2, follow = -2, acc = 0;
#pragma unroll
    for (int i = 0; i < NBANDS; i++) {
      float ly = lyb[w][h][i];
      ly = (float)MAX16(logMax - 8, MAX16(follow - 2.5, ly));
      logMax = MAX16(logMax, ly);
      follow = (float)MAX16(follow - 2.5, ly);
      acc += ly * dct[i * NBANDS + l];
    }
    float c = (float)(acc * sq);
    if (l == 0) c += -4;
    cpb[w][h][l] = c;
  }
  __syncthreads();
  /* burg_cepstral_analysis (freq.c:192-198), and the rest of a predictor row */
  if (live) {
    if (lane < NBANDS) {
      const float c0 = cpb[w][0][lane], c1 = cpb[w][1][lane];
      out[lane] = (float)(.5 * (c0 + c1));
      out[NBANDS + lane] = (c0 - c1);
    }
    if ((A.fill & BURG_FILL_ZERO) && l < NF && h == 1) out[BURG_N + l] = 0.f;
    if ((A.fill & BURG_FILL_FLAG) && lane == 63) out[PLC_IN - 1] = A.flag;
  }
}

__global__ void plc_row_fill_kernel(float *rows, float flag, const unsigned char *active, int nstreams)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int s = i / 64, c = i % 64;
  if (s >= nstreams || (active && !active[s])) return;
  if (c < BURG_N) rows[(size_t)s * PLC_IN + c] = 0.f;
  else if (c == PLC_IN - 1) rows[(size_t)s * PLC_IN + c] = flag;
}

int launch_burg(const BurgArgs &a, void *stream)
{
  if (a.nstreams < 1 || (!a.pcm && !a.pcm_f) || !a.out || a.stride < (a.fill ? PLC_IN : BURG_N) || !a.lpc_tab || !a.tab || !a.btab ||
      !a.cbuf || !a.xbuf || !a.obuf)
    return -1;
  const int grid = (a.nstreams + BS - 1) / BS;
  hipLaunchKernelGGL(burg_acf_kernel, dim3(grid), dim3(64 * BS), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(burg_rec_kernel, dim3((2 * a.nstreams + 63) / 64), dim3(64), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(burg_ceps_kernel, dim3(grid), dim3(64 * BS), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_plc_row_fill(float *rows, float flag, const unsigned char *active, int nstreams, void *stream)
{
  if (nstreams < 1 || !rows) return -1;
  const int grid = (nstreams * 64 + 255) / 256;
  hipLaunchKernelGGL(plc_row_fill_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, rows, flag, active, nstreams);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace lpcnet_mi355x
