/*
 * gru_tile.h -- compute_gruB (nnet.c:326-372, DOT_PROD / USE_SU_BIAS, a zero
 * condition) of one layer for a workgroup's tile of PLC_TILE = 16 streams on
 * v_mfma_i32_16x16x64_i8, shared by plc_kernel.hip and rdovae_kernel.hip.
 *
 * A wave owns unit tiles ut = wave, wave + 8, ...; per tile six accumulators
 * (z, r, h of the input product, K = inputs; z, r, h of the recurrent
 * product, K = units), each seeded from its half of subias, so lane l ends
 * with all six sums of units 16 ut + 4 (l / 16) + 0..3 of stream l % 16 and
 * runs their elementwise step in registers, in the C order of nnet.c:362-371.
 * The weights are the A tiles and seeds of side_kernels.h PlcArgs; x rows
 * are LDS bytes [stream][K + 16] (u8 ^ 0x80).  The caller puts a workgroup
 * barrier before (the rows are complete) and after (the outputs are).
 */
#ifndef LPCNET_GRU_TILE_H
#define LPCNET_GRU_TILE_H

#include "mf_common.h"
#include "side_kernels.h" /* PlcArgs, PLC_THREADS */

namespace lpcnet_mi355x {

/* compute_gruB of one layer for the workgroup's 16 streams: M inputs (xq,
 * row stride xs), N units (old state quantised in hq, row stride hs; floats
 * in st, the tile's first stream, row stride sstride).  xq_out (row stride
 * xos) takes the quantised new state, hf (row stride hfs) the new state as
 * floats; either may be null. */
template <bool HW>
__device__ __forceinline__ void plc_gru(int M, int N, const uint4 *Win, const uint4 *Wrec, const int *seed,
                                        const unsigned char *xq, int xs, const unsigned char *hq, int hs, float *st,
                                        int sstride, int nvalid, const unsigned char *act, unsigned char *xq_out,
                                        int xos, float *hf, int hfs, const uint32_t *rcp)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = lane & 15, q = lane >> 4;
  const int nki = M / 64, nkr = N / 64;
#pragma unroll 1
  for (int ut = wave; ut < N / 16; ut += PLC_THREADS / 64) {
    const int u = 16 * ut + 4 * q;
    v4i ai[3], ar[3];
#pragma unroll
    for (int g = 0; g < 3; g++) {
      ai[g] = *(const v4i *)&seed[g * N + u];
      ar[g] = *(const v4i *)&seed[3 * N + g * N + u];
    }
    const uint4 *wi = Win + (size_t)ut * 3 * nki * 64 + lane;
    for (int kt = 0; kt < nki; kt++) {
      const v4i x = *(const v4i *)(xq + s * xs + 64 * kt + 16 * q);
#pragma unroll
      for (int g = 0; g < 3; g++) {
        const uint4 w = wi[(g * nki + kt) * 64];
        ai[g] = mfma16(v4i{(int)w.x, (int)w.y, (int)w.z, (int)w.w}, x, ai[g]);
      }
    }
    const uint4 *wr = Wrec + (size_t)ut * 3 * nkr * 64 + lane;
    for (int kt = 0; kt < nkr; kt++) {
      const v4i x = *(const v4i *)(hq + s * hs + 64 * kt + 16 * q);
#pragma unroll
      for (int g = 0; g < 3; g++) {
        const uint4 w = wr[(g * nkr + kt) * 64];
        ar[g] = mfma16(v4i{(int)w.x, (int)w.y, (int)w.z, (int)w.w}, x, ar[g]);
      }
    }
    float old[4] = {0.f, 0.f, 0.f, 0.f};
    if (s < nvalid) {
      const float4 t = *(const float4 *)&st[(size_t)s * sstride + u];
      old[0] = t.x; old[1] = t.y; old[2] = t.z; old[3] = t.w;
    }
    /* nnet.c:362-371: zrh[0..2N) += recur, sigmoid, h += recur_h * r, tanh,
     * z * state + (1 - z) * h; every sum converted with * SCALE_1 first
     * (vec_avx.h:751-753, 852-854) */
    float zr[8], h[4], nw[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      zr[i] = (float)ai[0][i] * kScale1 + (float)ar[0][i] * kScale1;
      zr[4 + i] = (float)ai[1][i] * kScale1 + (float)ar[1][i] * kScale1;
    }
    sigmoid_x86_n<8, HW>(zr, rcp);
#pragma unroll
    for (int i = 0; i < 4; i++) h[i] = (float)ai[2][i] * kScale1 + ((float)ar[2][i] * kScale1) * zr[4 + i];
    tanh_x86_n<4, HW>(h, rcp);
#pragma unroll
    for (int i = 0; i < 4; i++) nw[i] = zr[i] * old[i] + (1.f - zr[i]) * h[i];
    if (act[s]) *(float4 *)&st[(size_t)s * sstride + u] = make_float4(nw[0], nw[1], nw[2], nw[3]);
    if (xq_out)
      *(uint32_t *)(xq_out + s * xos + u) =
          quant_s8(nw[0]) | (quant_s8(nw[1]) << 8) | (quant_s8(nw[2]) << 16) | (quant_s8(nw[3]) << 24);
    if (hf) {
#pragma unroll
      for (int i = 0; i < 4; i++) hf[s * hfs + u + i] = nw[i];
    }
  }
}

}  // namespace lpcnet_mi355x

#endif
