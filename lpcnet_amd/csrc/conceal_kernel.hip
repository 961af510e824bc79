/*
 * conceal_kernel.hip -- the glue of lpcnet_plc_update_causal and
 * lpcnet_plc_conceal_causal (lpcnet_plc.c:188-337) and of their non-causal
 * siblings (:339-492) between their network and analysis calls, for the
 * streams of an index list: the DC filter, the blend, the attenuation, the
 * st->pcm moves, the plc_copy ring, the FEC row fetch, the deferred-feature
 * push, the non-causal mode's reversal, backward blend, queue fill and
 * end-of-tick reorder, and the gather / scatter between the streams' rows and
 * the work order a partial-batch synthesis step runs on.
 * Elementwise: lane = sample (or feature column), except the two double
 * recursions of the DC filter, lane = stream.  Arithmetic is the reference's
 * expression by expression, with its types; the file is compiled without
 * contraction like every other (one fused a*b+c in dc_mem's recursion
 * changes the output).
 */
#include <hip/hip_runtime.h>

#include "side_kernels.h"

namespace lpcnet_mi355x {

namespace {

constexpr int HALF = FRAME / 2;
constexpr double DC_CONST = 0.003; /* lpcnet_plc.c:183 */
constexpr int MOVE_THREADS = 256;
constexpr int MOVE_REGS = 3;       /* MOVE_THREADS * MOVE_REGS >= the longest move, MAX_FEATURES_DELAY * FRAME + HALF */
constexpr int FEC_REGS = 8;        /* MOVE_THREADS * FEC_REGS >= CONCEAL_FEC_ROWS * NF */
static_assert(MOVE_THREADS * MOVE_REGS >= MAX_FEATURES_DELAY * FRAME + HALF, "a move fits one block's registers");
static_assert(MOVE_THREADS * FEC_REGS >= CONCEAL_FEC_ROWS * NF, "the FEC queue fits one block's registers");

__global__ __launch_bounds__(64) void dc_kernel(ConcealData d, const int *idx, int n, short *io, int mode)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int s = idx[k];
  short *pcm = io + (size_t)s * FRAME;
  short *lp = d.lp + (size_t)s * FRAME;
  double dc_mem = d.dc[2 * s], syn_dc = d.dc[2 * s + 1];
  if (mode == CONCEAL_DC_REMOVE) { /* :196-203 */
    dc_mem += syn_dc;
    d.delta[s] = (int)syn_dc;
    syn_dc = 0;
    for (int i = 0; i < FRAME; i++) {
      const short l = (short)(int)floor(.5 + dc_mem);
      dc_mem += DC_CONST * (pcm[i] - dc_mem);
      pcm[i] = (short)(pcm[i] - l);
      lp[i] = l;
    }
  } else if (mode == CONCEAL_DC_RESTORE) { /* :284-286 */
    for (int i = 0; i < FRAME; i++) pcm[i] = (short)(pcm[i] + lp[i]);
  } else if (mode == CONCEAL_DC_CONCEAL) { /* :331-334 */
    const int add = (int)floor(.5 + dc_mem);
    for (int i = 0; i < FRAME; i++) {
      syn_dc += DC_CONST * (pcm[i] - syn_dc);
      pcm[i] = (short)(pcm[i] + add);
    }
  } else if (mode == CONCEAL_DC_REMOVE_BAK || mode == CONCEAL_DC_REDO) {
    if (mode == CONCEAL_DC_REMOVE_BAK) { /* :356, :364-366 */
      d.delta[s] = (int)syn_dc;
      dc_mem += syn_dc;
      syn_dc = 0;
      d.mem_bak[s] = dc_mem;
    } else { /* :388-393 */
      const short *syn = d.pcm + (size_t)s * (d.buf + FRAME) + HALF;
      for (int i = 0; i < FRAME; i++) pcm[i] = (short)(pcm[i] + lp[i]);
      dc_mem = d.mem_bak[s];
      for (int i = 0; i < HALF; i++) syn_dc += DC_CONST * (syn[i] - syn_dc);
      dc_mem += syn_dc;
      d.delta[s] = (int)((double)d.delta[s] + syn_dc); /* int delta += a double */
      syn_dc = 0;
    }
    for (int i = 0; i < FRAME; i++) { /* :367-371, :394-398 */
      const short l = (short)(int)floor(.5 + dc_mem);
      dc_mem += DC_CONST * (pcm[i] - dc_mem);
      pcm[i] = (short)(pcm[i] - l);
      lp[i] = l;
    }
  } else { /* :480-488 */
    short *dc_buf = d.dc_buf + (size_t)s * HALF;
    const int dc = (int)floor(.5 + dc_mem);
    for (int i = mode == CONCEAL_DC_CONCEAL_HALF ? HALF : 0; i < FRAME; i++) syn_dc += DC_CONST * (pcm[i] - syn_dc);
    for (int i = 0; i < HALF; i++) {
      pcm[i] = (short)(pcm[i] + dc_buf[i]);
      pcm[HALF + i] = (short)(pcm[HALF + i] + dc);
      dc_buf[i] = (short)dc;
    }
  }
  d.dc[2 * s] = dc_mem;
  d.dc[2 * s + 1] = syn_dc;
}

__global__ __launch_bounds__(256) void dc_restore_delayed_kernel(ConcealData d, const int *idx, int n, short *io)
{
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const int k = g / HALF, i = g % HALF;
  if (k >= n) return;
  const int s = idx[k];
  short *pcm = io + (size_t)s * FRAME;
  const short *lp = d.lp + (size_t)s * FRAME;
  short *dc_buf = d.dc_buf + (size_t)s * HALF;
  pcm[i] = (short)(pcm[i] + dc_buf[i]);        /* :445 */
  pcm[HALF + i] = (short)(pcm[HALF + i] + lp[i]); /* :446 */
  dc_buf[i] = lp[HALF + i];                     /* :447 */
}

__global__ __launch_bounds__(256) void reverse_kernel(ConcealData d, const int *idx, int n, const short *io)
{
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const int k = g / FRAME, i = g % FRAME;
  if (k >= n) return;
  const int s = idx[k];
  d.rev[(size_t)s * FRAME + i] = io[(size_t)s * FRAME + FRAME - i - 1];
}

__global__ __launch_bounds__(256) void blend_back_kernel(ConcealData d, const int *idx, int n)
{
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const int k = g / HALF, i = g % HALF;
  if (k >= n) return;
  const int s = idx[k];
  short *p = d.pcm + (size_t)s * (d.buf + FRAME) + (FRAME - 1 - i);
  const float w = d.blend_w[i];
  /* st->pcm[159-i] = (int)floor(.5 + w*st->pcm[159-i] + (1-w)*(rev[i]+delta)): float products, double sums */
  const float a = w * (float)*p;
  const float c = (1.f - w) * (float)(d.rev[(size_t)s * FRAME + i] + d.delta[s]);
  *p = (short)(int)floor((.5 + (double)a) + (double)c);
}

__global__ __launch_bounds__(256) void queue_fill_kernel(ConcealData d, const int *idx, int n, const short *io)
{
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const int k = g / FRAME, i = g % FRAME;
  if (k >= n) return;
  const int s = idx[k];
  d.queued[(size_t)s * FRAME + i] = i < HALF ? d.pcm[(size_t)s * (d.buf + FRAME) + HALF + i] : io[(size_t)s * FRAME + i - HALF];
}

__global__ __launch_bounds__(256) void reorder_kernel(ConcealData d, const int *idx, int n, short *io)
{
  const int k = blockIdx.x, i = threadIdx.x;
  if (k >= n) return;
  const int s = idx[k];
  short *pcm = io + (size_t)s * FRAME;
  short *buf = d.pcm + (size_t)s * (d.buf + FRAME);
  const short in = i < FRAME ? pcm[i] : (short)0;      /* pcm_save: pcm stands unchanged since :373 / :399 */
  const short syn = i < HALF ? buf[HALF + i] : (short)0;
  __syncthreads(); /* every load before any store */
  if (i < HALF) {
    pcm[HALF + i] = in; /* :440 */
    pcm[i] = syn;       /* :441 */
  }
  if (i < FRAME) buf[i] = in; /* :442 */
}

__global__ __launch_bounds__(256) void export_kernel(ConcealData d, const int *idx, int n, short *dst, int dst_off, int src_off, int cnt)
{
  const int k = blockIdx.x, i = threadIdx.x;
  if (k >= n || i >= cnt) return;
  const int s = idx[k];
  dst[(size_t)s * FRAME + dst_off + i] = d.pcm[(size_t)s * (d.buf + FRAME) + src_off + i];
}

__global__ __launch_bounds__(256) void blend_kernel(ConcealData d, const int *idx, int n, short *io)
{
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const int k = g / HALF, i = g % HALF;
  if (k >= n) return;
  const int s = idx[k];
  short *pcm = io + (size_t)s * FRAME;
  const float w = d.blend_w[i];
  /* pcm[i] = (int)floor(.5 + w*pcm[i] + (1-w)*(tmp[i]-delta)): float products, double sums */
  const float a = w * (float)pcm[i];
  const float c = (1.f - w) * (float)(d.tmp[(size_t)s * HALF + i] - d.delta[s]);
  pcm[i] = (short)(int)floor((.5 + (double)a) + (double)c);
}

__global__ __launch_bounds__(64) void attenuate_kernel(ConcealData d, const int *idx, int n, int loss_count)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const float att_table[10] = {0, 0, -.2f, -.2f, -.4f, -.4f, -.8f, -.8f, -1.6f, -1.6f}; /* :292 */
  float *f = d.features + (size_t)idx[k] * NF;
  float v;
  if (loss_count >= 10) v = (f[0] + att_table[9]) - (float)(2 * (loss_count - 9));
  else v = f[0] + att_table[loss_count];
  f[0] = -10.f > v ? -10.f : v; /* MAX16(-10, v) */
}

__global__ __launch_bounds__(MOVE_THREADS) void move_kernel(ConcealData d, const int *idx, int n, const short *io, int dst_off,
                                                            int src_buf, int src_off, int cnt)
{
  const int k = blockIdx.x;
  if (k >= n) return;
  const int s = idx[k];
  short *buf = d.pcm + (size_t)s * (d.buf + FRAME);
  const short *src = (src_buf ? buf : io + (size_t)s * FRAME) + src_off;
  short v[MOVE_REGS];
  for (int j = 0; j < MOVE_REGS; j++) {
    const int i = threadIdx.x + j * MOVE_THREADS;
    v[j] = i < cnt ? src[i] : (short)0;
  }
  __syncthreads(); /* RNN_MOVE: every load before any store */
  for (int j = 0; j < MOVE_REGS; j++) {
    const int i = threadIdx.x + j * MOVE_THREADS;
    if (i < cnt) buf[dst_off + i] = v[j];
  }
}

__global__ __launch_bounds__(256) void plc_push_kernel(ConcealData d, const int *idx, int n)
{
  const int k = blockIdx.x;
  if (k >= n) return;
  const int s = idx[k];
  float *copy = d.copy + (size_t)s * (d.delay + 1) * d.nt;
  const float *net = d.plc_state + (size_t)s * d.nt;
  /* element e of every copy is this thread's: the ring moves without a barrier */
  for (int e = threadIdx.x; e < d.nt; e += blockDim.x) {
    for (int j = d.delay; j > 0; j--) copy[(size_t)j * d.nt + e] = copy[(size_t)(j - 1) * d.nt + e];
    copy[e] = net[e];
  }
}

__global__ __launch_bounds__(256) void plc_restore_kernel(ConcealData d, const int *idx, int n, int which)
{
  const int k = blockIdx.x;
  if (k >= n) return;
  const int s = idx[k];
  const float *copy = d.copy + ((size_t)s * (d.delay + 1) + which) * d.nt;
  float *net = d.plc_state + (size_t)s * d.nt;
  for (int e = threadIdx.x; e < d.nt; e += blockDim.x) net[e] = copy[e];
}

__global__ __launch_bounds__(256) void fec_fetch_kernel(ConcealData d, const int *idx, int n, int pos)
{
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const int k = g / 64, c = g % 64;
  if (k >= n || c >= PLC_IN) return;
  const int s = idx[k];
  float v = 0.f;
  if (c >= 2 * NBANDS && c < 2 * NBANDS + NF) {
    v = d.fec[((size_t)s * CONCEAL_FEC_ROWS + pos) * NF + (c - 2 * NBANDS)];
    d.features[(size_t)s * NF + (c - 2 * NBANDS)] = v;
  } else if (c == PLC_IN - 1) {
    v = -1.f;
  }
  d.rows[(size_t)s * PLC_IN + c] = v;
}

__global__ __launch_bounds__(256) void defer_push_kernel(ConcealData d, const int *idx, int n, int analysed, int fill)
{
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const int k = g / 32, c = g % 32;
  if (k >= n || c >= NF) return;
  const int s = idx[k];
  const float v = analysed ? d.rows[(size_t)s * PLC_IN + 2 * NBANDS + c] : d.features[(size_t)s * NF + c];
  float *q = d.defer + (size_t)s * CONCEAL_DEFER * NF;
  if (fill == CONCEAL_DEFER) { /* lpcnet.c:126-127: column c of every row is this thread's */
    for (int r = 0; r + 1 < CONCEAL_DEFER; r++) q[r * NF + c] = q[(r + 1) * NF + c];
    q[(CONCEAL_DEFER - 1) * NF + c] = v;
  } else {
    q[fill * NF + c] = v;
  }
}

__global__ __launch_bounds__(256) void gather_kernel(const int *idx, int n, float *w_feat, const float *feat, int feat_stride, short *w_pcm,
                                                     const short *pcm, int pcm_stride, int N)
{
  const int k = blockIdx.x;
  if (k >= n) return;
  const int s = idx[k], t = threadIdx.x;
  if (w_feat && t < NF) w_feat[(size_t)k * NF + t] = feat[(size_t)s * feat_stride + t];
  if (w_pcm && t < N) w_pcm[(size_t)k * N + t] = pcm[(size_t)s * pcm_stride + t];
}

__global__ __launch_bounds__(256) void scatter_kernel(const int *idx, int n, const short *w_pcm, short *dst, int dst_stride, int N)
{
  const int k = blockIdx.x, t = threadIdx.x;
  if (k >= n || t >= N) return;
  dst[(size_t)idx[k] * dst_stride + t] = w_pcm[(size_t)k * N + t];
}

__global__ __launch_bounds__(256) void reset_signal_kernel(StreamState *st, const int *idx, int n, int ulaw0)
{
  const int k = blockIdx.x;
  if (k >= n) return;
  StreamState &x = st[idx[k]];
  for (int e = threadIdx.x; e < NA; e += blockDim.x) x.gru_a_state[e] = 0.f;
  if (threadIdx.x < NB) x.gru_b_state[threadIdx.x] = 0.f;
  if (threadIdx.x < NLPC) x.last_sig[threadIdx.x] = 0.f;
  if (threadIdx.x == 0) {
    x.deemph_mem = 0.f;
    x.last_exc = ulaw0;
  }
}

__global__ __launch_bounds__(MOVE_THREADS) void fec_compact_kernel(ConcealData d, int s, int from, int rows)
{
  float *q = d.fec + (size_t)s * CONCEAL_FEC_ROWS * NF;
  const int cnt = rows * NF;
  float v[FEC_REGS];
  for (int j = 0; j < FEC_REGS; j++) {
    const int i = threadIdx.x + j * MOVE_THREADS;
    v[j] = i < cnt ? q[from * NF + i] : 0.f;
  }
  __syncthreads();
  for (int j = 0; j < FEC_REGS; j++) {
    const int i = threadIdx.x + j * MOVE_THREADS;
    if (i < cnt) q[i] = v[j];
  }
}

struct FecRow {
  float v[NF];
};

__global__ __launch_bounds__(64) void fec_store_kernel(ConcealData d, int s, int pos, FecRow r)
{
  if (threadIdx.x < NF) d.fec[((size_t)s * CONCEAL_FEC_ROWS + pos) * NF + threadIdx.x] = r.v[threadIdx.x];
}

int launched() { return hipGetLastError() == hipSuccess ? 0 : -1; }

int blocks(size_t lanes, int threads) { return (int)((lanes + threads - 1) / threads); }

}  // namespace

int launch_conceal_dc(const ConcealData &d, const int *idx, int n, short *io, int mode, void *stream)
{
  if (n <= 0) return 0;
  if (!idx || !io || mode < CONCEAL_DC_REMOVE || mode > CONCEAL_DC_CONCEAL_WHOLE) return -1;
  if (mode > CONCEAL_DC_CONCEAL && (!d.mem_bak || !d.dc_buf)) return -1;
  hipLaunchKernelGGL(dc_kernel, dim3(blocks(n, 64)), dim3(64), 0, (hipStream_t)stream, d, idx, n, io, mode);
  return launched();
}

int launch_conceal_blend(const ConcealData &d, const int *idx, int n, short *io, void *stream)
{
  if (n <= 0) return 0;
  if (!idx || !io) return -1;
  hipLaunchKernelGGL(blend_kernel, dim3(blocks((size_t)n * HALF, 256)), dim3(256), 0, (hipStream_t)stream, d, idx, n, io);
  return launched();
}

int launch_conceal_attenuate(const ConcealData &d, const int *idx, int n, int loss_count, void *stream)
{
  if (n <= 0) return 0;
  if (!idx || loss_count < 0) return -1;
  hipLaunchKernelGGL(attenuate_kernel, dim3(blocks(n, 64)), dim3(64), 0, (hipStream_t)stream, d, idx, n, loss_count);
  return launched();
}

int launch_conceal_move(const ConcealData &d, const int *idx, int n, const short *io, int dst_off, int src_buf, int src_off, int cnt,
                        void *stream)
{
  if (n <= 0 || cnt == 0) return 0;
  const int size = d.buf + FRAME;
  if (!idx || cnt < 0 || cnt > MOVE_THREADS * MOVE_REGS || dst_off < 0 || dst_off + cnt > size || src_off < 0 ||
      src_off + cnt > (src_buf ? size : FRAME) || (!src_buf && !io))
    return -1;
  hipLaunchKernelGGL(move_kernel, dim3(n), dim3(MOVE_THREADS), 0, (hipStream_t)stream, d, idx, n, io, dst_off, src_buf, src_off, cnt);
  return launched();
}

int launch_conceal_plc_push(const ConcealData &d, const int *idx, int n, void *stream)
{
  if (n <= 0) return 0;
  if (!idx) return -1;
  hipLaunchKernelGGL(plc_push_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, d, idx, n);
  return launched();
}

int launch_conceal_plc_restore(const ConcealData &d, const int *idx, int n, int k, void *stream)
{
  if (n <= 0) return 0;
  if (!idx || k < 0 || k > d.delay) return -1;
  hipLaunchKernelGGL(plc_restore_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, d, idx, n, k);
  return launched();
}

int launch_conceal_fec_fetch(const ConcealData &d, const int *idx, int n, int pos, void *stream)
{
  if (n <= 0) return 0;
  if (!idx || pos < 0 || pos >= CONCEAL_FEC_ROWS) return -1;
  hipLaunchKernelGGL(fec_fetch_kernel, dim3(blocks((size_t)n * 64, 256)), dim3(256), 0, (hipStream_t)stream, d, idx, n, pos);
  return launched();
}

int launch_conceal_defer_push(const ConcealData &d, const int *idx, int n, int analysed, int fill, void *stream)
{
  if (n <= 0) return 0;
  if (!idx || fill < 0 || fill > CONCEAL_DEFER) return -1;
  hipLaunchKernelGGL(defer_push_kernel, dim3(blocks((size_t)n * 32, 256)), dim3(256), 0, (hipStream_t)stream, d, idx, n, analysed,
                     fill);
  return launched();
}

int launch_conceal_gather_rows(const int *idx, int n, float *w_feat, const float *feat, int feat_stride, short *w_pcm, const short *pcm,
                               int pcm_stride, int N, void *stream)
{
  if (n <= 0 || (!w_feat && !w_pcm)) return 0;
  if (!idx || (w_feat && (!feat || feat_stride < NF)) || (w_pcm && (!pcm || N < 1 || N > FRAME || pcm_stride < N))) return -1;
  hipLaunchKernelGGL(gather_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, idx, n, w_feat, feat, feat_stride, w_pcm, pcm, pcm_stride,
                     N);
  return launched();
}

int launch_conceal_scatter_rows(const int *idx, int n, const short *w_pcm, short *dst, int dst_stride, int N, void *stream)
{
  if (n <= 0) return 0;
  if (!idx || !w_pcm || !dst || N < 1 || N > FRAME || dst_stride < N) return -1;
  hipLaunchKernelGGL(scatter_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, idx, n, w_pcm, dst, dst_stride, N);
  return launched();
}

int launch_conceal_dc_restore_delayed(const ConcealData &d, const int *idx, int n, short *io, void *stream)
{
  if (n <= 0) return 0;
  if (!idx || !io || !d.dc_buf) return -1;
  hipLaunchKernelGGL(dc_restore_delayed_kernel, dim3(blocks((size_t)n * HALF, 256)), dim3(256), 0, (hipStream_t)stream, d, idx, n, io);
  return launched();
}

int launch_conceal_reverse(const ConcealData &d, const int *idx, int n, const short *io, void *stream)
{
  if (n <= 0) return 0;
  if (!idx || !io || !d.rev) return -1;
  hipLaunchKernelGGL(reverse_kernel, dim3(blocks((size_t)n * FRAME, 256)), dim3(256), 0, (hipStream_t)stream, d, idx, n, io);
  return launched();
}

int launch_conceal_blend_back(const ConcealData &d, const int *idx, int n, void *stream)
{
  if (n <= 0) return 0;
  if (!idx || !d.rev || d.buf < 0) return -1;
  hipLaunchKernelGGL(blend_back_kernel, dim3(blocks((size_t)n * HALF, 256)), dim3(256), 0, (hipStream_t)stream, d, idx, n);
  return launched();
}

int launch_conceal_queue_fill(const ConcealData &d, const int *idx, int n, const short *io, void *stream)
{
  if (n <= 0) return 0;
  if (!idx || !io || !d.queued) return -1;
  hipLaunchKernelGGL(queue_fill_kernel, dim3(blocks((size_t)n * FRAME, 256)), dim3(256), 0, (hipStream_t)stream, d, idx, n, io);
  return launched();
}

int launch_conceal_reorder(const ConcealData &d, const int *idx, int n, short *io, void *stream)
{
  if (n <= 0) return 0;
  if (!idx || !io) return -1;
  hipLaunchKernelGGL(reorder_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, d, idx, n, io);
  return launched();
}

int launch_conceal_export(const ConcealData &d, const int *idx, int n, short *dst, int dst_off, int src_off, int cnt, void *stream)
{
  if (n <= 0) return 0;
  if (!idx || !dst || cnt < 1 || cnt > 256 || dst_off < 0 || dst_off + cnt > FRAME || src_off < 0 || src_off + cnt > d.buf + FRAME) return -1;
  hipLaunchKernelGGL(export_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, d, idx, n, dst, dst_off, src_off, cnt);
  return launched();
}

int launch_conceal_reset_signal(StreamState *st, const int *idx, int n, int ulaw0, void *stream)
{
  if (n <= 0) return 0;
  if (!st || !idx) return -1;
  hipLaunchKernelGGL(reset_signal_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, st, idx, n, ulaw0);
  return launched();
}

int launch_conceal_fec_compact(const ConcealData &d, int s, int from, int rows, void *stream)
{
  if (rows <= 0) return 0;
  if (s < 0 || s >= d.nstreams || from < 1 || from + rows > CONCEAL_FEC_ROWS) return -1;
  hipLaunchKernelGGL(fec_compact_kernel, dim3(1), dim3(MOVE_THREADS), 0, (hipStream_t)stream, d, s, from, rows);
  return launched();
}

int launch_conceal_fec_store(const ConcealData &d, int s, int pos, const float *features, void *stream)
{
  if (s < 0 || s >= d.nstreams || pos < 0 || pos >= CONCEAL_FEC_ROWS || !features) return -1;
  FecRow r;
  for (int i = 0; i < NF; i++) r.v[i] = features[i];
  hipLaunchKernelGGL(fec_store_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, d, s, pos, r);
  return launched();
}

}  // namespace lpcnet_mi355x
