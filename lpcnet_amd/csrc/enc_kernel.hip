/*
 * enc_kernel.hip -- process_superframe (lpcnet_enc.c:579-743) of the 1.6 kb/s
 * encoder for every stream of a batch, after feat_kernel<true> has run
 * compute_frame_features on the packet's four frames:
 *
 *   enc_pitch_kernel  the Viterbi pass over xc[2..9] and its backtrack
 *                     (:602-645; one wave per stream, lane per state, as
 *                     feat_kernel's single-frame pass), the pitch regression
 *                     and its quantisation (:650-697) and c0 (:704-706)
 *   enc_vq_kernel     quantize_3stage_mbest (:133-241), quantize_diff
 *                     (:283-318), double_interp_search (:379-400),
 *                     perform_double_interp (common.c:36-65), bits_pack
 *                     (:443-463, 724-733)
 *   enc_out_kernel    the live streams' rows into the caller's features
 *
 * Every float expression is the reference's, in its order; must be compiled
 * with -ffp-contract=off.  Each distance is d += (x[j]-c[j])*(x[j]-c[j]) in j
 * order on one lane: the parallelism is over codebook entries (lane = entry)
 * and streams.  The searches keep the reference's order: the five smallest
 * by (distance, index) for vq_quantize_mbest, the first minimum with the
 * positive-sign pass first for find_nearest_multi, the first minimum for
 * interp_search; the survivor merges are restated literally on one lane.
 * Distances of 1e15f or more and NaN are outside the contract
 * (lpcnet_engine.h, EncArgs).
 *
 * enc_vq_kernel: lane = entry.  A workgroup of 8 waves loads one codebook
 * stage (1024 x 17 floats, 70 KB) or an eighth of the difference codebook
 * (512 x 18 of 4096 x 18: its 295 KB do not fit the CU's 160 KB of LDS) and
 * every wave walks ENC_WAVE_STREAMS streams over it, 16 or 8 entries to a
 * lane; an odd row stride keeps a wave's reads off each other's banks.  Two
 * workgroups (75 KB of LDS each at one stream per wave) share a CU, so one
 * loads while the other searches.
 */
#include <hip/hip_runtime.h>

#include "device_math.h"
#include "side_kernels.h"
#include "lpc_stages.h"

namespace lpcnet_mi355x {

namespace {

/* streams per wave of enc_vq_kernel (streams per workgroup = 8 x this): 1
 * measured fastest (1 / 2 / 4: enc_kernel.hip's 0.194 / 0.346 / 0.652 ms per
 * packet at 1,024 streams, 1.89 / 2.83 / 2.77 at 32,768; tools/enc_bench.py,
 * DESIGN.md section 4 "enc_kernel") */
#ifndef ENC_WAVE_STREAMS
#define ENC_WAVE_STREAMS 1
#endif
constexpr int PS = 4;                 /* enc_pitch_kernel: streams (waves) per workgroup, as feat_kernel */
constexpr int NST = PITCH_STATES;
constexpr int NB1 = NBANDS - 1;       /* freq.h:49 NB_BANDS_1 */
constexpr int VW = 8;                 /* enc_vq_kernel: waves per workgroup */
constexpr int SPW = ENC_WAVE_STREAMS;
constexpr int VS = VW * SPW;          /* streams per workgroup */
constexpr int CB_N = 1024;            /* entries of a stage */
constexpr int CB_R = CB_N / 64;       /* entries per lane */
constexpr int DQ_N = 512;             /* entries of the difference codebook in LDS at a time */
constexpr int DQ_R = DQ_N / 64;
constexpr int DQ_PARTS = 4096 / DQ_N;
constexpr int DSTRIDE = NBANDS + 1;   /* LDS row stride of the difference codebook (odd) */
constexpr int CB_LDS = CB_N * NB1 > DQ_N * DSTRIDE ? CB_N * NB1 : DQ_N * DSTRIDE;
constexpr int SURV = 5;               /* SURVIVORS */
constexpr int FORBIDDEN = 7;          /* lpcnet_private.h:23 FORBIDDEN_INTERP */

}  // namespace

__global__ __launch_bounds__(64 * PS) void enc_pitch_kernel(EncArgs A)
{
  __shared__ float xcb[PS][8][PITCH_MAX];
  __shared__ float pmpb[PS][PITCH_MAX];
  __shared__ unsigned char prevb[PS][8][NST];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int sid = blockIdx.x * PS + w;
  const bool live = sid < A.nstreams && (!A.active || A.active[sid]); /* wave-uniform */
  const int s0 = live ? sid : 0;
  FeatState *S = A.state + s0;
  float(*xc)[PITCH_MAX] = xcb[w];
  float *pmp = pmpb[w];

  /* frame_weight[2..9] normalised (lpcnet_enc.c:602-603), on every lane */
  float fw[8];
  {
    float sum = 1e-15f;
#pragma unroll
    for (int sub = 0; sub < 8; sub++) {
      fw[sub] = live ? A.fw[(size_t)s0 * 8 + sub] : 0.f;
      sum += fw[sub];
    }
#pragma unroll
    for (int sub = 0; sub < 8; sub++) fw[sub] *= (8.f / sum);
  }
  if (live) {
#pragma unroll
    for (int sub = 0; sub < 8; sub++)
#pragma unroll
      for (int t = 0; t < 4; t++) xc[sub][lane + 64 * t] = A.xc[((size_t)s0 * 8 + sub) * PITCH_MAX + lane + 64 * t];
    for (int k = lane; k < PITCH_MAX; k += 64) pmp[k] = S->pitch_max_path[k];
  }
  __syncthreads();
  /* the sub-harmonic check (:607-610): every read before any write (lpc_stages.h) */
  for (int sub = 0; sub < 8; sub++) {
    float nv[3];
    if (live) subharmonic_row(xc[sub], lane, nv);
    __syncthreads();
    if (live)
#pragma unroll
      for (int t = 0; t < 3; t++) xc[sub][lane + 64 * t] = nv[t];
  }
  __syncthreads();

  /* the forward pass (:604-635), as feat_kernel's over two rows */
  float max_all = live ? S->pitch_max_path_all : 0.f;
  int best_i = live ? S->best_i : 0;
  for (int sub = 0; sub < 8; sub++) viterbi_step(live, lane, pmp, xc[sub], fw[sub], prevb[w][sub], max_all, best_i);
  if (!live) return; /* no barrier below */

  for (int k = lane; k < NST; k += 64) S->pitch_max_path[k] = pmp[k];
  const size_t fs = (size_t)A.nstreams * NF; /* next frame of this stream */
  float *feat = A.feat + (size_t)sid * NF;
  if (!A.quantize && lane < NBANDS) A.vq_mem[(size_t)sid * NBANDS + lane] = feat[3 * fs + lane]; /* :719 */
  if (lane != 0) return;
  S->pitch_max_path_all = max_all;
  S->best_i = best_i;

  /* backward pass (:636-645) */
  int best[10];
  float frame_corr = 0;
  {
    int bi = best_i;
    for (int sub = 7; sub >= 0; sub--) {
      best[2 + sub] = PITCH_MAX - bi;
      frame_corr += fw[sub] * xc[sub][bi];
      bi = prevb[w][sub][bi];
    }
  }
  frame_corr /= 8;
  if (!A.quantize) {
    for (int sub = 0; sub < 4; sub++) {
      int p = best[2 + 2 * sub] + best[2 + 2 * sub + 1];
      p = p < 510 ? p : 510;
      p = p > 66 ? p : 66;
      feat[sub * fs + NBANDS] = .01f * (p - 200);
      feat[sub * fs + NBANDS + 1] = frame_corr - .5f;
    }
    return;
  }
  if (frame_corr < 0) frame_corr = 0;
  /* the pitch contour (:650-675): float sums in the order written */
  float sx = 0, sxx = 0, sxy = 0, sy = 0, sw = 0;
  for (int sub = 2; sub < 10; sub++) {
    const float wt = fw[sub - 2];
    sw += wt;
    sx += wt * sub;
    sxx += wt * sub * sub;
    sxy += wt * sub * best[sub];
    sy += wt * best[sub];
  }
  const bool voiced = (double)frame_corr >= .3;
  float best_a = (sw * sxy - sx * sy) / (sw * sxx - sx * sx);
  int corr_id;
  if (voiced) {
    const float mean_pitch = sy / sw;
    const float max_a = mean_pitch / 32;
    const float lo = MAX16(-max_a, best_a);
    best_a = MIN16(max_a, lo);
    corr_id = cvtt_f64(floor((double)((frame_corr - .3f) / .175f)));
    frame_corr = 0.3875f + .175f * corr_id;
  } else {
    best_a = 0;
    corr_id = cvtt_f64(floor((double)(frame_corr / .075f)));
    frame_corr = 0.0375f + .075f * corr_id;
  }
  const float best_b = (sy - best_a * sx) / sw;
  /* "main" pitch + slope (:677-681); silence: sw = 0, best_b = NaN, both casts INT_MIN */
  const float center_pitch = best_b + 5.5f * best_a;
  const int main_pitch = enc_main_pitch(A.tab->pitch_thr, center_pitch);
  int modulation = cvtt_f64(floor(.5 + (double)(16 * 7 * best_a / center_pitch)));
  modulation = modulation < 3 ? modulation : 3;
  modulation = modulation > -3 ? modulation : -3;
  for (int sub = 0; sub < 4; sub++) {
    float p = A.pitch[main_pitch]; /* (float)(pow(2.f, main_pitch/21.)*PITCH_MIN_PERIOD) */
    p *= 1.f + modulation / 16.f / 7.f * (2 * sub - 3);
    const float lo = MAX16(33, p);
    p = MIN16(255, lo);
    feat[sub * fs + NBANDS] = .02f * (p - 100);
    feat[sub * fs + NBANDS + 1] = frame_corr - .5f;
  }
  /* c0 (:704-706) */
  int c0_id = cvtt_f64(floor(.5 + (double)(feat[3 * fs] * 4)));
  c0_id = c0_id < 63 ? c0_id : 63;
  c0_id = c0_id > -64 ? c0_id : -64;
  feat[3 * fs] = c0_id / 4.f;
  int *fl = A.fields + (size_t)sid * 4;
  fl[0] = c0_id + 64;
  fl[1] = main_pitch;
  fl[2] = voiced ? modulation + 4 : 0;
  fl[3] = corr_id;
}

namespace {

/* what one lane of a wave wrote to LDS stands for the others */
__device__ __forceinline__ void wave_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

/* vq_quantize_mbest (lpcnet_enc.c:53-78) of the stage in LDS, mbest = 5: the
 * five smallest by (distance, index), the same on every lane.  The serial
 * loop's strict < puts an equal distance after the earlier index, which is
 * this order. */
__device__ __forceinline__ void search5(const float *cb, int lane, const float *x, float (&d5)[SURV], int (&i5)[SURV])
{
  float d[CB_R];
#pragma unroll
  for (int r = 0; r < CB_R; r++) d[r] = 0;
  /* one band at a time: unrolled over the bands as well, the reads of all
   * 272 values are hoisted and spill */
#pragma unroll 1
  for (int j = 0; j < NB1; j++) {
    const float xj = x[j];
#pragma unroll
    for (int r = 0; r < CB_R; r++) {
      const float t = xj - cb[(lane + 64 * r) * NB1 + j];
      d[r] += t * t;
    }
  }
  float pd = -1.f; /* below every distance */
  int pi = -1;
#pragma unroll
  for (int m = 0; m < SURV; m++) {
    float bd = __builtin_inff();
    int bi = 0;
#pragma unroll
    for (int r = 0; r < CB_R; r++) {
      const int i = lane + 64 * r;
      const bool after = d[r] > pd || (d[r] == pd && i > pi);
      if (after && d[r] < bd) { /* r ascending: the lane's first */
        bd = d[r];
        bi = i;
      }
    }
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
      const float od = __shfl_xor(bd, s, 64);
      const int oi = __shfl_xor(bi, s, 64);
      if (od < bd || (od == bd && oi < bi)) {
        bd = od;
        bi = oi;
      }
    }
    d5[m] = bd;
    i5[m] = bi;
    pd = bd;
    pi = bi;
  }
}

}  // namespace

__global__ __launch_bounds__(64 * VW) void enc_vq_kernel(EncArgs A)
{
  __shared__ __attribute__((aligned(16))) float cb[CB_LDS];
  __shared__ float fin[VS][4][NBANDS];  /* features[0..3][0..17]; [3][0] is quantised already */
  __shared__ float memb[VS][NBANDS];    /* vq_mem */
  __shared__ float f3q[VS][NBANDS], f1q[VS][NBANDS];
  __shared__ int sidx[VS][2][SURV][3];  /* the survivors' paths: the stage before, this stage */
  __shared__ float gdist[VS][SURV];
  __shared__ float xw[VW][4 * NBANDS];  /* a wave's search target: [NB1], or the four classes' [4][NBANDS] */
  __shared__ float wd[VW][SURV];
  __shared__ int wi[VW][SURV];
  __shared__ float bestd[VS];
  __shared__ int bestk[VS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const size_t fs = (size_t)A.nstreams * NF;
  bool live[SPW];
  int sids[SPW];
#pragma unroll
  for (int q = 0; q < SPW; q++) {
    sids[q] = blockIdx.x * VS + w + VW * q;
    live[q] = sids[q] < A.nstreams && (!A.active || A.active[sids[q]]); /* wave-uniform */
  }
#pragma unroll
  for (int q = 0; q < SPW; q++)
    if (live[q]) {
      const int s = w + VW * q;
      for (int e = lane; e < 4 * NBANDS; e += 64) fin[s][e / NBANDS][e % NBANDS] = A.feat[(e / NBANDS) * fs + (size_t)sids[q] * NF + e % NBANDS];
      if (lane < NBANDS) memb[s][lane] = A.vq_mem[(size_t)sids[q] * NBANDS + lane];
    }

  /* quantize_3stage_mbest (lpcnet_enc.c:133-241) */
  for (int c = 0; c < 3; c++) {
    const float *src = c == 0 ? A.cb1 : (c == 1 ? A.cb2 : A.cb3);
    __syncthreads(); /* the stage before is consumed; fin stands */
    for (int k = tid; k < CB_N * NB1 / 4; k += 64 * VW) ((float4 *)cb)[k] = ((const float4 *)src)[k];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < SPW; q++) {
      if (!live[q]) continue;
      const int s = w + VW * q;
      int(*prev)[3] = sidx[s][(c + 1) & 1];
      int(*cur)[3] = sidx[s][c & 1];
      float *gd = gdist[s];
      const int nk = c == 0 ? 1 : SURV;
      for (int k = 0; k < nk; k++) {
        /* the search's target (:144, 153, 186), a band to a lane */
        float *x = xw[w];
        wave_sync(); /* the search before has read x */
        if (lane < NB1) {
          float t = fin[s][3][1 + lane];
          if (c >= 1) t = t - A.cb1[prev[k][0] * NB1 + lane];
          if (c == 2) t = t - A.cb2[prev[k][1] * NB1 + lane];
          x[lane] = t;
        }
        wave_sync();
        float d5[SURV];
        int i5[SURV];
        search5(cb, lane, x, d5, i5);
        if (lane == 0) {
          /* the survivor merge (:146-148, 156-180, 189-216), literally: m
           * advances only on insertion */
#pragma unroll
          for (int m = 0; m < SURV; m++) {
            wd[w][m] = d5[m];
            wi[w][m] = i5[m];
          }
          if (k == 0) {
            for (int m = 0; m < SURV; m++) {
              for (int e = 0; e < c; e++) cur[m][e] = prev[0][e];
              cur[m][c] = wi[w][m];
              gd[m] = wd[w][m];
            }
          } else if (wd[w][0] < gd[SURV - 1]) {
            int m = 0;
            for (int pos = 0; pos < SURV; pos++) {
              if (wd[w][m] < gd[pos]) {
                for (int j = SURV - 1; j >= pos + 1; j--) {
                  gd[j] = gd[j - 1];
                  for (int e = 0; e <= c; e++) cur[j][e] = cur[j - 1][e];
                }
                gd[pos] = wd[w][m];
                for (int e = 0; e < c; e++) cur[pos][e] = prev[k][e];
                cur[pos][c] = wi[w][m];
                m++;
              }
            }
          }
        }
      }
    }
  }
  __syncthreads();
  /* features[3][1..17] (:218-231): the winning path is sidx[.][0][0] */
#pragma unroll
  for (int q = 0; q < SPW; q++)
    if (live[q] && lane < NBANDS) {
      const int s = w + VW * q;
      const int *e = sidx[s][0][0];
      f3q[s][lane] = lane == 0 ? fin[s][3][0]
                               : A.cb1[e[0] * NB1 + lane - 1] + A.cb2[e[1] * NB1 + lane - 1] + A.cb3[e[2] * NB1 + lane - 1];
    }

  /* quantize_diff (:283-318) with find_nearest_multi (:243-280), DQ_N
   * entries of the codebook at a time: entry i's class i & 3 is the lane's,
   * lane & 3 */
  for (int qt = 0; qt < DQ_PARTS; qt++) {
    __syncthreads(); /* the part before is consumed; f3q stands */
    for (int k = tid; k < DQ_N * NBANDS; k += 64 * VW) cb[(k / NBANDS) * DSTRIDE + k % NBANDS] = A.cbd[(size_t)qt * DQ_N * NBANDS + k];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < SPW; q++) {
      if (!live[q]) continue;
      const int s = w + VW * q;
      /* target[class][band] (:294-297) */
      float *tg = xw[w];
      wave_sync();
      for (int e = lane; e < 4 * NBANDS; e += 64) {
        const int cl = e / NBANDS, j = e % NBANDS;
        const float left = memb[s][j], right = f3q[s][j];
        const float pred = cl < 2 ? .5f * (left + right) : (cl == 2 ? left : right);
        tg[e] = fin[s][1][j] - pred;
      }
      wave_sync();
      const float *tl = tg + (lane & 3) * NBANDS;
      float dp[DQ_R], dn[DQ_R];
#pragma unroll
      for (int r = 0; r < DQ_R; r++) dp[r] = dn[r] = 0;
#pragma unroll 1
      for (int j = 0; j < NBANDS; j++) {
        const float tj = tl[j];
#pragma unroll
        for (int r = 0; r < DQ_R; r++) {
          const float cv = cb[(lane + 64 * r) * DSTRIDE + j];
          const float a = tj - cv, b = tj + cv;
          dp[r] += a * a;
          dn[r] += b * b;
        }
      }
      /* the serial order: the positive pass, then the negative, i ascending;
       * strict <: the first minimum, by (distance, pass, index) */
      float bd = __builtin_inff();
      int bk = 0;
#pragma unroll
      for (int r = 0; r < DQ_R; r++)
        if (dp[r] < bd) {
          bd = dp[r];
          bk = qt * DQ_N + lane + 64 * r;
        }
#pragma unroll
      for (int r = 0; r < DQ_R; r++)
        if (dn[r] < bd) {
          bd = dn[r];
          bk = 4096 + qt * DQ_N + lane + 64 * r;
        }
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) {
        const float od = __shfl_xor(bd, m, 64);
        const int ok = __shfl_xor(bk, m, 64);
        if (od < bd || (od == bd && ok < bk)) {
          bd = od;
          bk = ok;
        }
      }
      if (lane == 0 && (qt == 0 || bd < bestd[s] || (bd == bestd[s] && bk < bestk[s]))) {
        bestd[s] = bd;
        bestk[s] = bk;
      }
    }
  }
  __syncthreads();
  /* features[1] (:300-307) */
#pragma unroll
  for (int q = 0; q < SPW; q++)
    if (live[q] && lane < NBANDS) {
      const int s = w + VW * q;
      int id = bestk[s];
      float sg = 1;
      if (id >= 4096) {
        sg = -1;
        id -= 4096;
      }
      const float left = memb[s][lane], right = f3q[s][lane];
      const int cls = id & 3;
      const float pred = cls < 2 ? .5f * (left + right) : (cls == 2 ? left : right);
      f1q[s][lane] = pred + sg * A.cbd[(size_t)id * NBANDS + lane];
    }
  __syncthreads();
  /* double_interp_search (:320-340, 379-400), perform_double_interp
   * (common.c:36-65), vq_mem (:719) and the packet (:724-733) */
#pragma unroll
  for (int q = 0; q < SPW; q++) {
    if (!live[q]) continue;
    const int s = w + VW * q, sid = sids[q];
    float dist = 0;
    if (lane < 6) {
      const int k = lane % 3 + 1, h = lane / 3;
      const float *x = fin[s][h ? 2 : 0], *left = h ? f1q[s] : memb[s], *right = h ? f3q[s] : f1q[s];
      for (int i = 0; i < NBANDS; i++) {
        const float pred = k == 1 ? .5f * (left[i] + right[i]) : (k == 2 ? left[i] : right[i]);
        dist += (x[i] - pred) * (x[i] - pred);
      }
    }
    float dd[6];
#pragma unroll
    for (int e = 0; e < 6; e++) dd[e] = __shfl(dist, e, 64);
    int best_id = 0;
    float min_dist = 1e15f;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const int id = 3 * i + j;
        const float d = dd[i] + dd[3 + j];
        if (d < min_dist && id != FORBIDDEN) {
          min_dist = d;
          best_id = id;
        }
      }
    const int interp_id = best_id - (best_id >= FORBIDDEN);
    const int id0 = best_id / 3, id1 = best_id % 3;
    if (lane < NBANDS) {
      const float mem = memb[s][lane], f1 = f1q[s][lane], f3 = f3q[s][lane];
      float *o = A.feat + (size_t)sid * NF + lane;
      o[0 * fs] = id0 == 0 ? .5f * (mem + f1) : (id0 == 1 ? mem : f1);
      o[1 * fs] = f1;
      o[2 * fs] = id1 == 0 ? .5f * (f1 + f3) : (id1 == 1 ? f1 : f3);
      o[3 * fs] = f3;
      A.vq_mem[(size_t)sid * NBANDS + lane] = f3;
    }
    if (lane == 0 && A.packets) {
      /* bits_pack keeps the low nb_bits of each field, MSB first */
      const int *fl = A.fields + (size_t)sid * 4;
      const int *e = sidx[s][0][0];
      unsigned long long v = 0;
      auto put = [&](unsigned data, int n) { v = (v << n) | (data & ((1u << n) - 1)); };
      put((unsigned)fl[0], 7);
      put((unsigned)fl[1], 6);
      put((unsigned)fl[2], 3);
      put((unsigned)fl[3], 2);
      put((unsigned)e[0], 10);
      put((unsigned)e[1], 10);
      put((unsigned)e[2], 10);
      put((unsigned)bestk[s], 13);
      put((unsigned)interp_id, 3);
      unsigned char *buf = A.packets + (size_t)sid * 8;
#pragma unroll
      for (int k = 0; k < 8; k++) buf[k] = (unsigned char)(v >> (56 - 8 * k));
    }
  }
}

/* the live streams' st->features: feat [4][B][NF] | lpc [4][B][NLPC] ->
 * features [4][B][row]; one thread per value */
__global__ __launch_bounds__(256) void enc_out_kernel(EncArgs A)
{
  const size_t n = (size_t)4 * A.nstreams * A.row;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int j = (int)(t % A.row);
  const size_t ks = t / A.row; /* frame * B + stream */
  const int sid = (int)(ks % A.nstreams);
  if (A.active && !A.active[sid]) return;
  A.features[t] = j < NF ? A.feat[ks * NF + j] : A.lpc[ks * NLPC + j - NF];
}

int launch_enc_pitch(const EncArgs &a, void *stream)
{
  if (a.nstreams < 1 || !a.state || !a.vq_mem || !a.xc || !a.fw || !a.feat || !a.fields || !a.tab || (a.quantize && !a.pitch)) return -1;
  hipLaunchKernelGGL(enc_pitch_kernel, dim3((a.nstreams + PS - 1) / PS), dim3(64 * PS), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_enc_vq(const EncArgs &a, void *stream)
{
  if (a.nstreams < 1 || !a.vq_mem || !a.feat || !a.fields || !a.cb1 || !a.cb2 || !a.cb3 || !a.cbd) return -1;
  hipLaunchKernelGGL(enc_vq_kernel, dim3((a.nstreams + VS - 1) / VS), dim3(64 * VW), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_enc_out(const EncArgs &a, void *stream)
{
  if (a.nstreams < 1 || !a.features || !a.feat || !a.lpc || (a.row != NF && a.row != NTF)) return -1;
  const size_t n = (size_t)4 * a.nstreams * a.row;
  hipLaunchKernelGGL(enc_out_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace lpcnet_mi355x
