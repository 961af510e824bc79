/*
 * lpc_kernel.hip -- lpc_from_cepstrum (freq.c:310-320) for every stream of a
 * batch on the GPU: one wavefront per stream, eight streams per workgroup.
 *
 * Restates, term for term and in the reference's operation order:
 *   idct                 freq.c:230-240   lanes 0..17, one band each
 *   pow(10, Ex)*comp     freq.c:318       pow10_dd.h (double-double, exact
 *                                         against glibc: pow10_exhaustive.c)
 *   interp_band_gain     freq.c:202-216   lane per spectrum bin
 *   inverse_transform    freq.c:256-273   Opus kiss FFT, 320 points, factors
 *                                         4,4,4,5 (kiss_fft.c:101-305, 518-586):
 *                                         one lane per butterfly, LDS between
 *                                         stages, digit-reversed scaled input
 *   lpc_from_bands       freq.c:275-297   noise floor + lag window (double)
 *   lpcn_lpc             freq.c:86-127    Levinson-Durbin, float build, lane 0
 * The stages live in lpc_stages.h, which feat_kernel.hip, burg_kernel.hip and
 * enc_kernel.hip share.
 * Must be compiled with -ffp-contract=off.  The output feeds the frame
 * kernel's two-frame LPC ring (lpcnet.c:110-112), so this kernel is two
 * frames ahead of its first use.
 */
#include <hip/hip_runtime.h>

#include "side_kernels.h"
#include "lpc_stages.h"

namespace lpcnet_mi355x {

namespace {

constexpr int WIN = LPC_WIN; /* NBANDS (lpcnet_engine.h) == LPC_NBANDS */
#ifndef LPC_WG_STREAMS
#define LPC_WG_STREAMS 8
#endif
constexpr int LPC_STREAMS = LPC_WG_STREAMS; /* streams (waves) per workgroup */

}  // namespace

/* the warm-up of the next tick's chunk kernel weights (deferred form): the
 * workgroups of an XCD (workgroup b runs on XCD b % 8) split every line of
 * the matrices and touch it once; the XOR only keeps the loads alive */
__device__ __forceinline__ void l2_warm_lines(const L2Warm &W)
{
  const int x = blockIdx.x % 8, nx = ((int)gridDim.x - 1 - x) / 8 + 1, k = blockIdx.x / 8;
  uint32_t acc = 0;
#pragma unroll
  for (int t = 0; t < 5; t++)
    for (int o = k * (int)blockDim.x + (int)threadIdx.x; o < W.lines[t]; o += nx * (int)blockDim.x)
      acc ^= W.m[t][(size_t)o * 32];
  asm volatile("" ::"v"(acc));
}

__global__ __launch_bounds__(64 * LPC_STREAMS) void lpc_kernel(const float *features, float *lpc_out, int nstreams,
                                                               const LpcTables *T, StreamState *ring, int ring_depth,
                                                               L2Warm warm)
{
  if (warm.m[0]) l2_warm_lines(warm); /* issued first, in flight under the LPC work */
  __shared__ C2 ybuf[LPC_STREAMS][WIN];
  __shared__ C2 tw[WIN];
  __shared__ float dct[NBANDS * NBANDS];
  __shared__ LpcSlot slot[WIN];
  __shared__ float Eb[LPC_STREAMS][NBANDS + 2];
  __shared__ float acb[LPC_STREAMS][LPC_ORDER1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int sid = blockIdx.x * LPC_STREAMS + w;
  const bool live = sid < nstreams; /* wave-uniform */
  /* every global read up front (one round of latency): this stream's
   * cepstrum, then the tables into LDS */
  float ceps[NBANDS];
  if (live && lane < NBANDS) {
    const float *c = features + (size_t)sid * NF;
#pragma unroll
    for (int j = 0; j < NBANDS; j++) ceps[j] = c[j];
  }
  stage_fft_dct<true>(T, tw, dct, slot);
  const double sq = T->sqrt_2_18;
  const float cmp = lane < NBANDS ? T->comp[lane] : 0.f, scale = T->scale;
  C2 *y = ybuf[w];
  float *E = Eb[w];
  __syncthreads();

  /* idct, band powers, interpolated spectrum, inverse FFT, windowed
   * autocorrelation (lpc_stages.h) */
  lpc_autocorr_stages(live, lane, ceps, y, E, acb[w], LpcLds{tw, dct, slot, sq, cmp, scale});

  /* Levinson-Durbin, float build of lpcn_lpc (freq.c:86-127): one lane
   * per stream of the workgroup, all in wave 0 (the recursion is serial: one
   * lane of each wave would issue it four times); fully unrolled, so lpc[]
   * and ac[] stay in registers (a dynamic index into a register array costs
   * a select chain per access) */
  const int lsid = blockIdx.x * LPC_STREAMS + lane;
  if (w == 0 && lane < LPC_STREAMS && lsid < nstreams) {
    float lpc[LPC_ORDER1 - 1];
    levinson16(acb[lane], lpc);
    if (ring) {
      /* deferred form (one-frame ticks, FEATURES_DELAY >= 1): push this
       * frame's LPC into the stream's ring (lpcnet.c:110-114: the oldest slot
       * was read by the frame's chunk_kernel already) */
      float4 *q = (float4 *)ring[lsid].old_lpc[0];
      for (int j = ring_depth - 1; j > 0; j--)
#pragma unroll
        for (int i = 0; i < NLPC / 4; i++) q[j * (NLPC / 4) + i] = q[(j - 1) * (NLPC / 4) + i];
#pragma unroll
      for (int i = 0; i < NLPC / 4; i++) q[i] = make_float4(lpc[4 * i], lpc[4 * i + 1], lpc[4 * i + 2], lpc[4 * i + 3]);
      return;
    }
    float4 *o = (float4 *)(lpc_out + (size_t)lsid * NLPC);
#pragma unroll
    for (int i = 0; i < NLPC / 4; i++) o[i] = make_float4(lpc[4 * i], lpc[4 * i + 1], lpc[4 * i + 2], lpc[4 * i + 3]);
  }
}

int launch_lpc(const float *features, float *lpc_out, int nstreams, const LpcTables *tables, void *stream,
               StreamState *ring, int ring_depth, const L2Warm *warm)
{
  if (ring && (ring_depth < 1 || ring_depth > MAX_FEATURES_DELAY)) return -1;
  const int grid = (nstreams + LPC_STREAMS - 1) / LPC_STREAMS;
  L2Warm w{};
  if (warm) w = *warm;
  hipLaunchKernelGGL(lpc_kernel, dim3(grid), dim3(64 * LPC_STREAMS), 0, (hipStream_t)stream, features, lpc_out, nstreams,
                     tables, ring, ring_depth, w);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace lpcnet_mi355x
