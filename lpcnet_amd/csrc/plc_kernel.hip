/*
 * plc_kernel.hip -- the PLC prediction network (compute_plc_pred,
 * src/lpcnet_plc.c:135-145) for every stream of a batch in one launch.
 *
 *   plc_dense1  57 -> cond, tanh            (_lpcnet_compute_dense, sgemv_accum16)
 *   plc_gru1    cond -> n1                  (compute_gruB, nnet.c:326-372)
 *   plc_gru2    n1 -> n2                    (compute_gruB)
 *   plc_out     n2 -> 20, linear            (the generic loop of sgemv_accum, nnet.c:80-84)
 *   out[19] = MIN16(.5f, out[19] + .1f)
 *
 * The one place in the engine where the batch makes a GEMM: one weight set,
 * M = streams.  A 512-thread workgroup owns a tile of PLC_TILE = 16 streams,
 * the N of v_mfma_i32_16x16x64_i8 (mf_common.h mfma16: A = 16 weight rows,
 * B = 16 streams, 64 k per instruction, exact int32 sums).
 *
 * Phases (a workgroup barrier between two):
 *   0  the tile's inputs -> LDS floats; both GRU states quantised -> LDS bytes
 *   1  dense1: a thread owns one output row for 4 streams, bias then one FMA
 *      per input column in index order, tanh, quantised -> LDS bytes
 *   2  GRU1 (plc_gru, gru_tile.h, shared with rdovae_kernel.hip): a wave owns
 *      unit tiles ut = wave, wave + 8, ...; per tile six
 *      accumulators (z, r, h of the input product, K = inputs; z, r, h of the
 *      recurrent product, K = units), each seeded from its half of subias, so
 *      lane l ends with all six sums of units 16 ut + 4 (l / 16) + 0..3 of
 *      stream l % 16 and runs their elementwise step in registers, in the C
 *      order of nnet.c:362-371; new state -> global, quantised -> LDS (GRU2's
 *      input)
 *   3  GRU2 the same; new state -> global and, as floats, -> LDS
 *   4  plc_out: a thread owns one (stream, row), bias then a separate multiply
 *      and add per column in index order; the out[19] boost
 *
 * LDS: x rows are [stream][K + 16] bytes (u8 ^ 0x80 = u8 - 128, what the
 * signed product consumes; 128 * rowsum(w) is in the seed): lane l reads the
 * 16 bytes at 64 kt + 16 (l / 16) of stream l % 16 with one ds_read_b128; the
 * 16-byte row padding spreads the 16 streams over the banks.  The operand that
 * streams is the weights: [ut][gate][kt][64 lanes] uint4 in global memory, one
 * coalesced 1 KiB read per MFMA, shared by every workgroup through L2
 * (0.7 MB for the default shape).
 *
 * Numerics: SURVEY.md Appendix A items 1-4 and 6; activations are the general
 * tanh_x86_n / sigmoid_x86_n of device_math.h in the hardware-reciprocal (HW)
 * or the table form, chosen per launch from the batch's rcpps table.
 * Out of scope: int8 weights whose maddubs pairs can saturate (the host
 * refuses such a model: trained PLC models are clipped against it) and an
 * fp32 predictor.
 * Compile with -ffp-contract=off.
 */
#include "gru_tile.h"

namespace lpcnet_mi355x {

namespace {

/* byte offsets of the LDS sections */
struct PlcLds {
  int in, act, xq1, hq1, xq2, hq2, hf, total;
  int xs1, hs1, xs2, hs2, hfs; /* row strides: bytes (x rows), floats (hf) */
};

__host__ __device__ inline PlcLds plc_lds(int C, int N1, int N2)
{
  PlcLds L;
  L.xs1 = C + 16;
  L.hs1 = N1 + 16;
  L.xs2 = N1 + 16;
  L.hs2 = N2 + 16;
  L.hfs = N2 + 1;
  L.in = 0;
  L.act = L.in + PLC_TILE * PLC_IN * 4;
  L.xq1 = L.act + 16;
  L.hq1 = L.xq1 + PLC_TILE * L.xs1;
  L.xq2 = L.hq1 + PLC_TILE * L.hs1;
  L.hq2 = L.xq2 + PLC_TILE * L.xs2;
  L.hf = L.hq2 + PLC_TILE * L.hs2;
  L.total = L.hf + PLC_TILE * L.hfs * 4;
  return L;
}

template <bool HW>
__global__ __launch_bounds__(PLC_THREADS) void plc_kernel(PlcArgs A)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char plc_smem[];
  const int C = A.cond, N1 = A.n1, N2 = A.n2, NT = N1 + N2;
  const PlcLds L = plc_lds(C, N1, N2);
  float *in_l = (float *)(plc_smem + L.in);
  unsigned char *act = plc_smem + L.act;
  unsigned char *xq1 = plc_smem + L.xq1, *hq1 = plc_smem + L.hq1, *xq2 = plc_smem + L.xq2, *hq2 = plc_smem + L.hq2;
  float *hf = (float *)(plc_smem + L.hf);
  const int tid = threadIdx.x;
  const int s0 = blockIdx.x * PLC_TILE;
  const int nvalid = min(PLC_TILE, A.nstreams - s0);
  float *st = A.state + (size_t)s0 * NT;

  /* phase 0 */
  if (tid < PLC_TILE) act[tid] = tid < nvalid && (!A.active || A.active[s0 + tid] != 0) ? 1 : 0;
  for (int idx = tid; idx < PLC_TILE * PLC_IN; idx += PLC_THREADS) {
    const int s = idx / PLC_IN;
    in_l[idx] = A.in && s < nvalid ? A.in[(size_t)s0 * PLC_IN + idx] : 0.f;
  }
  for (int idx = tid; idx < PLC_TILE * NT; idx += PLC_THREADS) {
    const int s = idx / NT, k = idx - s * NT;
    const float v = s < nvalid ? st[idx] : 0.f;
    const unsigned char b = (unsigned char)quant_s8(v);
    if (k < N1) hq1[s * L.hs1 + k] = b;
    else hq2[s * L.hs2 + k - N1] = b;
  }
  __syncthreads();

  /* phase 1: plc_dense1 */
  for (int idx = tid; idx < C * (PLC_TILE / 4); idx += PLC_THREADS) {
    const int sg = idx / C, row = idx - sg * C;
    const float *x = in_l + 4 * sg * PLC_IN;
    float a[4];
    const float bias = A.d1_b[row];
#pragma unroll
    for (int k = 0; k < 4; k++) a[k] = bias;
#pragma unroll 3
    for (int j = 0; j < PLC_IN; j++) {
      const float w = A.d1_w[j * C + row];
#pragma unroll
      for (int k = 0; k < 4; k++) a[k] = __builtin_fmaf(w, x[k * PLC_IN + j], a[k]);
    }
    tanh_x86_n<4, HW>(a, A.rcp);
#pragma unroll
    for (int k = 0; k < 4; k++) xq1[(4 * sg + k) * L.xs1 + row] = (unsigned char)quant_s8(a[k]);
  }
  __syncthreads();

  /* phase 2, 3: plc_gru1, plc_gru2 */
  plc_gru<HW>(C, N1, A.g1_in, A.g1_rec, A.g1_seed, xq1, L.xs1, hq1, L.hs1, st, NT, nvalid, act, xq2, L.xs2, nullptr, 0,
              A.rcp);
  __syncthreads();
  plc_gru<HW>(N1, N2, A.g2_in, A.g2_rec, A.g2_seed, xq2, L.xs2, hq2, L.hs2, st + N1, NT, nvalid, act, nullptr, 0, hf,
              L.hfs, A.rcp);
  __syncthreads();

  /* phase 4: plc_out and the correlation boost */
  if (!A.out) return;
  for (int idx = tid; idx < PLC_TILE * NF; idx += PLC_THREADS) {
    const int s = idx / NF, i = idx - s * NF;
    float o = A.out_b[i];
    const float *x = hf + s * L.hfs;
#pragma unroll 8
    for (int j = 0; j < N2; j++) o = o + A.out_w[j * NF + i] * x[j];
    if (i == NF - 1) {
      const float v = o + .1f;
      o = .5f < v ? .5f : v; /* MIN16(.5f, out[19] + .1f) */
    }
    if (act[s]) A.out[(size_t)(s0 + s) * NF + i] = o;
  }
}

}  // namespace

int plc_lds_bytes(int cond, int n1, int n2) { return plc_lds(cond, n1, n2).total; }

int launch_plc(const PlcArgs &a, void *stream)
{
  if (a.nstreams <= 0) return 0;
  const int lds = plc_lds_bytes(a.cond, a.n1, a.n2);
  const int grid = (a.nstreams + PLC_TILE - 1) / PLC_TILE;
  if (a.rcp_hw) {
    if (ensure_dyn_lds((const void *)plc_kernel<true>, lds)) return -1;
    hipLaunchKernelGGL(plc_kernel<true>, dim3(grid), dim3(PLC_THREADS), lds, (hipStream_t)stream, a);
  } else {
    if (ensure_dyn_lds((const void *)plc_kernel<false>, lds)) return -1;
    hipLaunchKernelGGL(plc_kernel<false>, dim3(grid), dim3(PLC_THREADS), lds, (hipStream_t)stream, a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace lpcnet_mi355x
