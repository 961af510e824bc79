/*
 * rdovae_kernel.hip -- the DRED RDO-VAE encoder and decoder
 * (dred_rdovae_enc.c:38-95 dred_rdovae_encode_dframe, dred_rdovae_dec.c:37-98
 * dec_init_states / decode_qframe, dred_rdovae.c:38-52 DRED_rdovae_decode_all)
 * for every stream of a batch in one launch.
 *
 *   stack   dense1 (tanh) -> GRU2 -> dense3 -> GRU4 -> dense5 -> GRU6 ->
 *           dense7 -> dense8, every output appended to one concatenation of
 *           T floats
 *   encode  the stack on 2 x 20 features; latents = bits_dense (causal conv,
 *           linear) over the conv memory and the concatenation; initial
 *           state = gdense2(gdense1(concatenation)), both tanh
 *   decode  dec_init: the three GRU states = state1..3(initial state), tanh;
 *           qframe: the stack on a latent, then dec_final (linear) over the
 *           concatenation -> 80 floats; decode_all: init and every qframe of
 *           a packet in one launch on a scratch state
 *
 * A 512-thread workgroup owns a tile of PLC_TILE = 16 streams, as in
 * plc_kernel.hip, with a workgroup barrier between layers.
 *   GRUs    plc_gru of gru_tile.h: v_mfma_i32_16x16x64_i8 over the shared A
 *           tiles, quantised activations as LDS byte rows, the elementwise
 *           step in registers
 *   dense, conv
 *           a thread owns one output row for 4 streams: bias, then the columns
 *           in index order.  rows % 16 == 0 is sgemv_accum16 (one FMA per
 *           column), any other row count the generic loop of sgemv_accum
 *           (nnet.c:73-86: a separate multiply and add per column).  The k of
 *           a chain is never split across lanes.
 *
 * LDS: two float rows [stream][wmax + 1] (a layer's input and output), the
 * GRU input bytes [stream][K + 16] and the three GRUs' quantised states.  The
 * concatenation is not in LDS: at T = 2048 it is 128 KiB for 16 streams,
 * which with the rows above leaves no room in a CU's 160 KiB.  It is a
 * per-tile scratch in global memory, [T][16 streams] so that a head reads the
 * 4 streams of a column with one 16-byte load; each layer writes its part
 * once and the heads read it once, from L2 (DESIGN.md has the reasoning).
 * The conv reads the (ksize - 1) T floats of per-stream memory from global
 * memory and writes the shifted memory back.
 *
 * Inactive streams (active[s] == 0) and the padding streams of a partial tile
 * leave state, memory and output rows untouched.
 *
 * Numerics: as plc_kernel.hip; activations are
 * tanh_x86_n / sigmoid_x86_n in the HW or the table form, per launch.
 * Out of scope: the statistical model (the dred_*_q8 / q10 / q15 tables,
 * which the blob does not carry) and any entropy coding of latents; an fp32
 * RDO-VAE; emulating maddubs saturation (the host refuses such weights);
 * writing decoded frames into the concealment machine's FEC ring on the
 * device; training and export.
 * Compile with -ffp-contract=off.
 */
#include "gru_tile.h"

namespace lpcnet_mi355x {

namespace {

struct RdoLds {
  int act, fa, fb, xq, hq[3], total;
  int ws, qs, hs[3]; /* row strides: floats (fa, fb), bytes */
};

__host__ __device__ inline RdoLds rdo_lds(const RdovaeNet &n)
{
  RdoLds L;
  L.ws = n.wmax + 1;
  int qmax = 0;
  for (int k = 0; k < 3; k++) {
    qmax = n.g[k].in > qmax ? n.g[k].in : qmax;
    L.hs[k] = n.g[k].n + 16;
  }
  L.qs = qmax + 16;
  L.act = 0;
  L.fa = 16;
  L.fb = L.fa + PLC_TILE * L.ws * 4;
  L.xq = (L.fb + PLC_TILE * L.ws * 4 + 15) & ~15;
  L.hq[0] = L.xq + PLC_TILE * L.qs;
  L.hq[1] = L.hq[0] + PLC_TILE * L.hs[0];
  L.hq[2] = L.hq[1] + PLC_TILE * L.hs[1];
  L.total = L.hq[2] + PLC_TILE * L.hs[2];
  return L;
}

/* `cols` columns of a thread's chain: a[k] of stream 4 sg + k; w points at the
 * row's first weight, `rows` apart per column; x(j) gives the four streams'
 * value of column j.  Four columns' loads are in flight at once; deeper
 * unrolling was measured and not kept. */
template <bool FMA, class X>
__device__ __forceinline__ void chain(float (&a)[4], const float *w, int rows, int cols, X x)
{
#pragma unroll 4
  for (int j = 0; j < cols; j++) {
    const float wv = w[(size_t)j * rows];
    const float4 v = x(j);
    if (FMA) {
      a[0] = __builtin_fmaf(wv, v.x, a[0]);
      a[1] = __builtin_fmaf(wv, v.y, a[1]);
      a[2] = __builtin_fmaf(wv, v.z, a[2]);
      a[3] = __builtin_fmaf(wv, v.w, a[3]);
    } else {
      a[0] = a[0] + wv * v.x;
      a[1] = a[1] + wv * v.y;
      a[2] = a[2] + wv * v.z;
      a[3] = a[3] + wv * v.w;
    }
  }
}

/* where a dense layer's outputs go; any may be null */
struct DenseOut {
  float *lds = nullptr;         /* [stream][ls] floats */
  int ls = 0;
  unsigned char *q = nullptr;   /* [stream][qs] quantised */
  int qs = 0;
  float *cat = nullptr;         /* [row][PLC_TILE], at the layer's offset */
  float *g = nullptr;           /* global [stream][gs], the tile's first stream; active streams only */
  size_t gs = 0;
};

template <bool HW>
__device__ __forceinline__ void dense_store(const DenseOut &o, float (&a)[4], int row, int sg, bool tanh_act,
                                            const unsigned char *act, const uint32_t *rcp)
{
  if (tanh_act) tanh_x86_n<4, HW>(a, rcp);
  if (o.lds) {
#pragma unroll
    for (int k = 0; k < 4; k++) o.lds[(4 * sg + k) * o.ls + row] = a[k];
  }
  if (o.q) {
#pragma unroll
    for (int k = 0; k < 4; k++) o.q[(4 * sg + k) * o.qs + row] = (unsigned char)quant_s8(a[k]);
  }
  if (o.cat) *(float4 *)&o.cat[row * PLC_TILE + 4 * sg] = make_float4(a[0], a[1], a[2], a[3]);
  if (o.g) {
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (act[4 * sg + k]) o.g[(size_t)(4 * sg + k) * o.gs + row] = a[k];
  }
}

/* column loaders: LDS float rows; the concatenation scratch */
struct XLds {
  const float *x;
  int xs;
  __device__ __forceinline__ float4 operator()(int j) const
  {
    return make_float4(x[j], x[xs + j], x[2 * xs + j], x[3 * xs + j]);
  }
};
struct XCat {
  const float *c; /* at 4 sg */
  __device__ __forceinline__ float4 operator()(int j) const { return *(const float4 *)&c[(size_t)j * PLC_TILE]; }
};
/* the conv memory of four streams (a padding stream reads a live one's) */
struct XMem {
  const float *m[4];
  __device__ __forceinline__ float4 operator()(int j) const { return make_float4(m[0][j], m[1][j], m[2][j], m[3][j]); }
};

/* one item (row, 4 streams) of a dense layer over loader x */
template <bool HW, class X>
__device__ __forceinline__ void dense_item(const RdovaeDense &D, int row, int sg, X x, bool tanh_act, const DenseOut &o,
                                           const unsigned char *act, const uint32_t *rcp)
{
  float a[4];
  const float bias = D.b[row];
#pragma unroll
  for (int k = 0; k < 4; k++) a[k] = bias;
  if (D.out % 16 == 0) chain<true>(a, D.w + row, D.out, D.in, x);
  else chain<false>(a, D.w + row, D.out, D.in, x);
  dense_store<HW>(o, a, row, sg, tanh_act, act, rcp);
}

/* _lpcnet_compute_dense of the tile from LDS rows x (row stride xs) */
template <bool HW>
__device__ __forceinline__ void dense_lds(const RdovaeDense &D, const float *x, int xs, bool tanh_act, const DenseOut &o,
                                          const unsigned char *act, const uint32_t *rcp)
{
  for (int idx = threadIdx.x; idx < D.out * (PLC_TILE / 4); idx += PLC_THREADS) {
    const int sg = idx / D.out, row = idx - sg * D.out;
    dense_item<HW>(D, row, sg, XLds{x + 4 * sg * xs, xs}, tanh_act, o, act, rcp);
  }
}

/* _lpcnet_compute_dense of the tile over the concatenation */
template <bool HW>
__device__ __forceinline__ void dense_cat(const RdovaeDense &D, const float *cat, int first, bool tanh_act, const DenseOut &o,
                                          const unsigned char *act, const uint32_t *rcp)
{
  for (int idx = threadIdx.x - first; idx < D.out * (PLC_TILE / 4); idx += PLC_THREADS) {
    if (idx < 0) continue;
    const int sg = idx / D.out, row = idx - sg * D.out;
    dense_item<HW>(D, row, sg, XCat{cat + 4 * sg}, tanh_act, o, act, rcp);
  }
}

/* the GRU states of the tile, quantised, into the three hq rows */
__device__ __forceinline__ void quant_states(const RdovaeNet &N, const RdoLds &L, unsigned char *smem, const float *st, int nvalid)
{
  const int n0 = N.g[0].n, n1 = N.g[1].n;
  for (int idx = threadIdx.x; idx < PLC_TILE * N.nt; idx += PLC_THREADS) {
    const int s = idx / N.nt, k = idx - s * N.nt;
    const float v = s < nvalid ? st[idx] : 0.f;
    const unsigned char b = (unsigned char)quant_s8(v);
    if (k < n0) smem[L.hq[0] + s * L.hs[0] + k] = b;
    else if (k < n0 + n1) smem[L.hq[1] + s * L.hs[1] + k - n0] = b;
    else smem[L.hq[2] + s * L.hs[2] + k - n0 - n1] = b;
  }
}

/* The eight layers on the input rows in fa; the hq rows hold the quantised
 * states.  Ends behind a barrier: the concatenation is complete and dense8's
 * reads of fb are done. */
template <bool HW>
__device__ __forceinline__ void run_stack(const RdovaeArgs &A, const RdoLds &L, unsigned char *smem, float *st, float *cat,
                                          int nvalid)
{
  const RdovaeNet &N = A.net;
  float *fa = (float *)(smem + L.fa), *fb = (float *)(smem + L.fb);
  unsigned char *act = smem + L.act, *xq = smem + L.xq;
  int goff = 0;
  for (int l = 0; l < 3; l++) {
    DenseOut o;
    o.q = xq;
    o.qs = L.qs;
    o.cat = cat + (size_t)N.off[2 * l] * PLC_TILE;
    dense_lds<HW>(N.d[l], fa, L.ws, true, o, act, A.rcp);
    __syncthreads();
    const RdovaeGru &G = N.g[l];
    plc_gru<HW>(G.in, G.n, G.win, G.wrec, G.seed, xq, L.qs, smem + L.hq[l], L.hs[l], st + goff, N.nt, nvalid, act, nullptr, 0,
                fa, L.ws, A.rcp);
    __syncthreads();
    /* RNN_COPY(&buffer[output_index], state, N) */
    float *c = cat + (size_t)N.off[2 * l + 1] * PLC_TILE;
    for (int idx = threadIdx.x; idx < G.n * PLC_TILE; idx += PLC_THREADS) c[idx] = fa[(idx % PLC_TILE) * L.ws + idx / PLC_TILE];
    goff += G.n;
  }
  DenseOut o7;
  o7.lds = fb;
  o7.ls = L.ws;
  o7.cat = cat + (size_t)N.off[6] * PLC_TILE;
  dense_lds<HW>(N.d[3], fa, L.ws, true, o7, act, A.rcp);
  __syncthreads();
  DenseOut o8;
  o8.cat = cat + (size_t)N.off[7] * PLC_TILE;
  dense_lds<HW>(N.d[4], fb, L.ws, true, o8, act, A.rcp);
  __syncthreads();
}

template <bool HW>
__global__ __launch_bounds__(PLC_THREADS) void rdovae_kernel(RdovaeArgs A)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char rdo_smem[];
  const RdovaeNet &N = A.net;
  const RdoLds L = rdo_lds(N);
  float *fa = (float *)(rdo_smem + L.fa), *fb = (float *)(rdo_smem + L.fb);
  unsigned char *act = rdo_smem + L.act;
  const int tid = threadIdx.x;
  const int s0 = blockIdx.x * PLC_TILE;
  const int nvalid = min(PLC_TILE, A.nstreams - s0);
  float *st = A.state + (size_t)s0 * N.nt;
  float *cat = A.cat + (size_t)blockIdx.x * N.T * PLC_TILE;

  if (tid < PLC_TILE) act[tid] = tid < nvalid && (!A.active || A.active[s0 + tid] != 0) ? 1 : 0;

  if (!A.decoder) {
    /* the two feature frames, the earlier first; the quantised states */
    for (int idx = tid; idx < PLC_TILE * 2 * NF; idx += PLC_THREADS) {
      const int s = idx / (2 * NF), i = idx - s * 2 * NF, f = i / NF;
      fa[s * L.ws + i] = s < nvalid ? A.in[(size_t)(s0 + s) * A.in_stream + f * A.in_frame + (i - f * NF)] : 0.f;
    }
    quant_states(N, L, rdo_smem, st, nvalid);
    __syncthreads();
    run_stack<HW>(A, L, rdo_smem, st, cat, nvalid);

    /* compute_conv1d(bits_dense) over [memory | concatenation], and gdense1 */
    const RdovaeDense &C = N.head[0];
    const int nmem = (N.ksize - 1) * N.T;
    float *mem = A.mem + (size_t)s0 * nmem;
    const int nconv = C.out * (PLC_TILE / 4);
    for (int idx = tid; idx < nconv; idx += PLC_THREADS) {
      const int sg = idx / C.out, row = idx - sg * C.out;
      XMem xm;
#pragma unroll
      for (int k = 0; k < 4; k++) xm.m[k] = mem + (size_t)min(4 * sg + k, nvalid - 1) * nmem;
      float a[4];
      const float bias = C.b[row];
#pragma unroll
      for (int k = 0; k < 4; k++) a[k] = bias;
      if (C.out % 16 == 0) {
        chain<true>(a, C.w + row, C.out, nmem, xm);
        chain<true>(a, C.w + (size_t)nmem * C.out + row, C.out, N.T, XCat{cat + 4 * sg});
      } else {
        chain<false>(a, C.w + row, C.out, nmem, xm);
        chain<false>(a, C.w + (size_t)nmem * C.out + row, C.out, N.T, XCat{cat + 4 * sg});
      }
      DenseOut o;
      o.g = A.latents + (size_t)s0 * C.out;
      o.gs = C.out;
      dense_store<HW>(o, a, row, sg, false, act, A.rcp);
    }
    DenseOut o1;
    o1.lds = fb;
    o1.ls = L.ws;
    /* the threads the conv leaves idle take gdense1's first items */
    dense_cat<HW>(N.head[1], cat, nconv % PLC_THREADS, true, o1, act, A.rcp);
    __syncthreads();
    /* RNN_COPY(mem, &tmp[nb_inputs], ...): every element moves down one slot,
     * the concatenation becomes the newest; a thread owns position p of every
     * slot of a stream, so no element is read after it was overwritten */
    for (int idx = tid; idx < PLC_TILE * N.T; idx += PLC_THREADS) {
      const int p = idx / PLC_TILE, s = idx - p * PLC_TILE;
      if (!act[s]) continue;
      float *m = mem + (size_t)s * nmem + p;
      for (int k = 0; k + 2 < N.ksize; k++) m[(size_t)k * N.T] = m[(size_t)(k + 1) * N.T];
      if (N.ksize > 1) m[(size_t)(N.ksize - 2) * N.T] = cat[idx];
    }
    DenseOut o2;
    o2.g = A.init_state + (size_t)s0 * N.head[2].out;
    o2.gs = N.head[2].out;
    dense_lds<HW>(N.head[2], fb, L.ws, true, o2, act, A.rcp);
    return;
  }

  if (A.d_init) {
    /* dred_rdovae_dec_init_states */
    const int S = N.head[0].in;
    for (int idx = tid; idx < PLC_TILE * S; idx += PLC_THREADS) {
      const int s = idx / S, i = idx - s * S;
      fa[s * L.ws + i] = s < nvalid ? A.d_init[(size_t)(s0 + s) * S + i] : 0.f;
    }
    __syncthreads();
    int goff = 0;
    for (int k = 0; k < 3; k++) {
      DenseOut o;
      o.g = st + goff;
      o.gs = N.nt;
      dense_lds<HW>(N.head[k], fa, L.ws, true, o, act, A.rcp);
      goff += N.g[k].n;
    }
    __syncthreads();
  }
  for (int f = 0; f < A.nframes; f++) {
    /* dred_rdovae_decode_qframe */
    const int Ld = N.in_dim;
    for (int idx = tid; idx < PLC_TILE * Ld; idx += PLC_THREADS) {
      const int s = idx / Ld, i = idx - s * Ld;
      fa[s * L.ws + i] = s < nvalid ? A.d_lat[((size_t)(s0 + s) * A.nframes + f) * Ld + i] : 0.f;
    }
    quant_states(N, L, rdo_smem, st, nvalid);
    __syncthreads();
    run_stack<HW>(A, L, rdo_smem, st, cat, nvalid);
    DenseOut o;
    o.g = A.d_out + ((size_t)s0 * A.nframes + f) * RDOVAE_QFRAME;
    o.gs = (size_t)A.nframes * RDOVAE_QFRAME;
    dense_cat<HW>(N.head[3], cat, 0, false, o, act, A.rcp);
    __syncthreads(); /* the next qframe overwrites the concatenation */
  }
}

}  // namespace

int rdovae_lds_bytes(const RdovaeNet &n) { return rdo_lds(n).total; }

int launch_rdovae(const RdovaeArgs &a, void *stream)
{
  if (a.nstreams <= 0) return 0;
  const int lds = rdovae_lds_bytes(a.net);
  const int grid = (a.nstreams + PLC_TILE - 1) / PLC_TILE;
  if (a.rcp_hw) {
    if (ensure_dyn_lds((const void *)rdovae_kernel<true>, lds)) return -1;
    hipLaunchKernelGGL(rdovae_kernel<true>, dim3(grid), dim3(PLC_THREADS), lds, (hipStream_t)stream, a);
  } else {
    if (ensure_dyn_lds((const void *)rdovae_kernel<false>, lds)) return -1;
    hipLaunchKernelGGL(rdovae_kernel<false>, dim3(grid), dim3(PLC_THREADS), lds, (hipStream_t)stream, a);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace lpcnet_mi355x
