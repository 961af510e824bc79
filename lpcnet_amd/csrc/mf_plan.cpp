/*
 * mf_plan.cpp -- GRU_A planner and register-table builder of the
 * matrix-core kernels (host side, deterministic; see mf_plan.h).
 */
#include "mf_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>

namespace lpcnet_mi355x {

MfPlanParams mf_plan_params_from_env()
{
  MfPlanParams pp;
  if (const char *v = getenv("LPCNET_MF_ITERS")) { pp.iters_set = true; pp.iters = atoi(v); }
  if (const char *v = getenv("LPCNET_MF_SIMD_W")) { pp.simd_w_set = true; pp.simd_w = atoi(v); }
  if (const char *v = getenv("LPCNET_MF_HOSTED_F")) pp.hosted_f = atoi(v);
  if (const char *v = getenv("LPCNET_MF_PIECE_W")) pp.piece_w = atoi(v);
  if (const char *v = getenv("LPCNET_MF_CAPS"))
    pp.caps_set = sscanf(v, "%d,%d,%d,%d", &pp.caps[0], &pp.caps[1], &pp.caps[2], &pp.caps[3]) == 4;
  pp.force_split = getenv("LPCNET_MF_FORCE_SPLIT") != nullptr;
  return pp;
}

namespace {

/* mf_kernel GRU_A layout helpers.
 *
 * Unit blocks (8 units = one block row of each gate) are dealt to the six
 * GRU_A waves.  A wave runs as many 4x4x4 MFMA slots per gate as its
 * longest block row has blocks (rounded up to 4), so the assignment
 * decides both the padding and the balance between the two waves sharing
 * each SIMD (w, w+4; waves 2 and 3 share theirs with the samplers). */
int mf_wave_cost(const std::vector<std::vector<int>> &ga, const int *ub8)
{
  size_t mz = 0, mh = 0;
  for (int j = 0; j < 8; j++) {
    mz = std::max(mz, std::max(ga[ub8[j]].size(), ga[NA / 8 + ub8[j]].size()));
    mh = std::max(mh, ga[2 * (NA / 8) + ub8[j]].size());
  }
  return 8 * (int)((mz + 3) / 4) + 4 * (int)((mh + 3) / 4);
}

/* per-SIMD load of six GRU_A wave costs: waves 0/4 and 1/5 pair up; 2 and 3
 * pair with a sampler (its priority chain takes most of their SIMD: measured
 * ~74 cycles per slot there against ~27 per slot of a wave pair), weighted
 * simd_w tenths */
int mf_simd_score(const int *c, int simd_w)
{
  return std::max(std::max(c[0] + c[4], c[1] + c[5]), (simd_w * std::max(c[2], c[3])) / 10);
}

/* extra[w]: a fixed per-wave cost on top of its own rows (split models: the
 * hosted pieces) */
std::vector<int> mf_assign_unit_blocks(const std::vector<std::vector<int>> &ga, const int *extra, int iters, int simd_w)
{
  constexpr int NUB = NA / 8;
  std::vector<int> perm(NUB);
  /* start: unit blocks by descending z/r length, dealt in order */
  for (int u = 0; u < NUB; u++) perm[u] = u;
  auto zr = [&](int u) { return std::max(ga[u].size(), ga[NUB + u].size()); };
  std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return zr(a) > zr(b); });
  auto score = [&](const std::vector<int> &p, long &sum) {
    int c[SAMPLE_WAVES];
    sum = 0;
    for (int w = 0; w < SAMPLE_WAVES; w++) sum += (c[w] = mf_wave_cost(ga, &p[8 * w]) + (extra ? extra[w] : 0));
    return mf_simd_score(c, simd_w);
  };
  long best_sum;
  int best = score(perm, best_sum);
  uint32_t rng = 12345u;
  for (int it = 0; it < iters; it++) {
    rng = rng * 1664525u + 1013904223u;
    const int a = (rng >> 8) % NUB;
    rng = rng * 1664525u + 1013904223u;
    const int b = (rng >> 8) % NUB;
    if (a / 8 == b / 8) continue;
    std::swap(perm[a], perm[b]);
    long sum;
    const int sc = score(perm, sum);
    if (sc < best || (sc == best && sum <= best_sum)) {
      best = sc;
      best_sum = sum;
    } else {
      std::swap(perm[a], perm[b]);
    }
  }
  return perm;
}

/* the block rows of ga cut to at most cap[g] blocks per gate */
std::vector<std::vector<int>> mf_capped_rows(const std::vector<std::vector<int>> &ga, const int cap[3])
{
  constexpr int NUB = NA / 8;
  std::vector<std::vector<int>> own(ga.size());
  for (int g = 0; g < 3; g++)
    for (int u = 0; u < NUB; u++) {
      const std::vector<int> &v = ga[g * NUB + u];
      own[g * NUB + u].assign(v.begin(), v.begin() + std::min((int)v.size(), cap[g]));
    }
  return own;
}

/* Slot order of the 4 block rows one 32-lane LDS group reads in the same
 * ds_read_b32 (rows4[k]: input offsets of row k's blocks).  Input quad c of
 * stream m sits at dword c + 104 m, bank (c + 8 m) mod 32: quads of
 * different c mod 8 never share a bank, equal quads broadcast.  Each row's
 * blocks are matched to slots (Kuhn augmenting paths) so that every slot's
 * quads are bank-disjoint; blocks that cannot be placed so take any free
 * slot.  Empty positions (zero weights) read a quad another row reads in
 * that slot.  Integer sums do not depend on the order. */
void mf_bank_slots(const std::vector<int> *const rows4[4], int nslot, int slot_of[4][MF_HMAX], int cb_at[4][MF_HMAX])
{
  int owner[4][MF_HMAX];
  int cls[MF_HMAX][8];
  for (int t = 0; t < MF_HMAX; t++)
    for (int c = 0; c < 8; c++) cls[t][c] = -1;
  for (int k = 0; k < 4; k++)
    for (int t = 0; t < MF_HMAX; t++) owner[k][t] = -1;
  int order[4] = {0, 1, 2, 3};
  std::stable_sort(order, order + 4, [&](int a, int b) { return rows4[a]->size() > rows4[b]->size(); });
  for (int oi = 0; oi < 4; oi++) {
    const int k = order[oi];
    const std::vector<int> &row = *rows4[k];
    const int n = (int)row.size();
    auto ok = [&](int i, int t) {
      const int cb = row[i] / 4, c = cb & 7;
      return cls[t][c] < 0 || cls[t][c] == cb;
    };
    int match_slot[MF_HMAX];  /* slot -> item of this row */
    for (int t = 0; t < nslot; t++) match_slot[t] = -1;
    std::vector<int> item_slot(n, -1);
    for (int i = 0; i < n; i++) {
      bool seen[MF_HMAX] = {};
      std::function<bool(int)> aug = [&](int it) -> bool {
        for (int t = 0; t < nslot; t++) {
          if (seen[t] || !ok(it, t)) continue;
          seen[t] = true;
          if (match_slot[t] < 0 || aug(match_slot[t])) {
            match_slot[t] = it;
            item_slot[it] = t;
            return true;
          }
        }
        return false;
      };
      aug(i);
    }
    for (int i = 0; i < n; i++)
      if (item_slot[i] < 0)
        for (int t = 0; t < nslot; t++)
          if (match_slot[t] < 0) {
            match_slot[t] = i;
            item_slot[i] = t;
            break;
          }
    for (int i = 0; i < n; i++) {
      const int t = item_slot[i], cb = row[i] / 4;
      slot_of[k][i] = t;
      owner[k][t] = cb;
      if (cls[t][cb & 7] < 0) cls[t][cb & 7] = cb;
    }
  }
  for (int t = 0; t < nslot; t++) {
    int any = 0;
    for (int k = 0; k < 4; k++)
      if (owner[k][t] >= 0) { any = owner[k][t]; break; }
    for (int k = 0; k < 4; k++) cb_at[k][t] = owner[k][t] >= 0 ? owner[k][t] : any;
  }
}

/* blocks [t0, t1) of block row rb (-1: none) */
struct MfRowSpan {
  int rb = -1, t0 = 0, t1 = 0;
};

/* Fill slots [slot0, slot0 + nslot) of one wave's table wtab
 * [MF_LANE_U32][64] for lane groups 4 half .. 4 half + 3 from their row
 * spans: the 4 block rows read by one 32-lane LDS group, slot order chosen so
 * their x words fall in distinct banks (mf_bank_slots); weight words, then
 * the slots' column-block bytes. */
void mf_fill_half_wave(const std::vector<std::vector<int>> &ga, const std::vector<int> &ga_first, const int8_t *wa,
                       const MfRowSpan span[4], int half, int slot0, int nslot, uint32_t *wtab)
{
  std::vector<int> lists[4];
  for (int k = 0; k < 4; k++)
    if (span[k].rb >= 0) lists[k].assign(ga[span[k].rb].begin() + span[k].t0, ga[span[k].rb].begin() + span[k].t1);
  const std::vector<int> *rows4[4] = {&lists[0], &lists[1], &lists[2], &lists[3]};
  int slot_of[4][MF_HMAX], cb_at[4][MF_HMAX];
  mf_bank_slots(rows4, nslot, slot_of, cb_at);
  auto word = [&](int k, int l) -> uint32_t & { return wtab[(size_t)k * 64 + l]; };
  for (int k = 0; k < 4; k++)
    for (int r = 0; r < 8; r++) {
      const int l = 8 * (4 * half + k) + r;
      for (int t = 0; t < (int)lists[k].size(); t++)
        memcpy(&word(slot0 + slot_of[k][t], l), wa + 32 * (ga_first[span[k].rb] + span[k].t0 + t) + 4 * r, 4);
      for (int t = 0; t < nslot; t++) word(MF_GA + (slot0 + t) / 4, l) |= (uint32_t)cb_at[k][t] << (8 * ((slot0 + t) & 3));
    }
}

/* first slot of gate g in a lane's table */
int mf_gate_base(int g) { return g == 0 ? 0 : (g == 1 ? MF_ZMAX : 2 * MF_ZMAX); }

/* One candidate split (own caps T, piece sizes F) laid out: own rows ->
 * lane groups balanced together with the hosted pieces (which waves host z/r
 * and h pieces: every subset that holds them and fits the registers, scored
 * by the per-SIMD load), pieces -> lane groups of the hosting waves.
 * Returns the score (-1: does not fit). */
long mf_layout(const std::vector<std::vector<int>> &ga, MfPlan &P, const int T[3], const int F[3], int iters, int simd_w,
               const MfPlanParams &pp)
{
  constexpr int NUB = NA / 8, NLG = SAMPLE_WAVES * 8;
  P.own[0] = T[0];
  P.own[1] = T[1];
  P.own[2] = T[2];
  for (int g = 0; g < 3; g++) {
    P.pieces[g].clear();
    for (int u = 0; u < NUB; u++) {
      const int K = (int)ga[g * NUB + u].size();
      if (K > T[g] && F[g] <= 0) return -1;
      for (int t0 = T[g]; t0 < K; t0 += F[g]) P.pieces[g].push_back(MfPiece{u, t0, std::min(K, t0 + F[g])});
    }
    if ((int)P.pieces[g].size() > NLG) return -1;
  }
  const std::vector<std::vector<int>> own = mf_capped_rows(ga, T);
  const int npz = (int)std::max(P.pieces[0].size(), P.pieces[1].size()), nph = (int)P.pieces[2].size();
  const int npieces = (int)(P.pieces[0].size() + P.pieces[1].size() + P.pieces[2].size());
  int extra[SAMPLE_WAVES] = {};
  int mz = 0, mh = 0; /* hosting waves (bit masks) */
  long best = -1;
  if (pp.iters_set) iters = pp.iters;
  if (pp.simd_w_set) simd_w = pp.simd_w;
  /* hosted-piece merge cost of a wave, in MFMA slots: its partial sums'
   * LDS adds (per gate hosted) */
  const int host_zr = (pp.hosted_f * 2 * F[0]) / 10 + 2 * MF_HOST_ADD_SLOTS, host_h = (pp.hosted_f * F[2]) / 10 + MF_HOST_ADD_SLOTS;
  P.perm = mf_assign_unit_blocks(own, extra, iters, simd_w);
  for (int round = 0; round < 2; round++) {
    int c[SAMPLE_WAVES], gz[SAMPLE_WAVES], gh[SAMPLE_WAVES];
    for (int w = 0; w < SAMPLE_WAVES; w++) {
      c[w] = mf_wave_cost(own, &P.perm[8 * w]);
      size_t az = 0, ah = 0;
      for (int j = 0; j < 8; j++) {
        const int ub = P.perm[8 * w + j];
        az = std::max(az, std::max(own[ub].size(), own[NUB + ub].size()));
        ah = std::max(ah, own[2 * NUB + ub].size());
      }
      gz[w] = (int)(az + 3) / 4;
      gh[w] = (int)(ah + 3) / 4;
    }
    best = -1;
    for (int sz = 0; sz < (1 << SAMPLE_WAVES); sz++) {
      if (8 * __builtin_popcount(sz) < npz || (npz == 0 && sz)) continue;
      for (int sh = 0; sh < (1 << SAMPLE_WAVES); sh++) {
        if (8 * __builtin_popcount(sh) < nph || (nph == 0 && sh)) continue;
        int cc[SAMPLE_WAVES];
        bool ok = true;
        long sum = 0;
        for (int w = 0; w < SAMPLE_WAVES && ok; w++) {
          cc[w] = c[w];
          if (sz >> w & 1) {
            ok &= 4 * gz[w] + F[0] <= MF_ZMAX;
            cc[w] += host_zr;
          }
          if (sh >> w & 1) {
            ok &= 4 * gh[w] + F[2] <= MF_HMAX;
            cc[w] += host_h;
          }
          sum += cc[w];
        }
        if (!ok) continue;
        const long sc = ((long)mf_simd_score(cc, simd_w) + (long)pp.piece_w * npieces / 10) * 4096 + sum;
        if (best < 0 || sc < best) {
          best = sc;
          mz = sz;
          mh = sh;
        }
      }
    }
    if (best < 0) return -1;
    if (round == 1) break;
    /* re-balance the own rows around the hosting waves' extra load */
    for (int w = 0; w < SAMPLE_WAVES; w++) extra[w] = (mz >> w & 1 ? host_zr : 0) + (mh >> w & 1 ? host_h : 0);
    P.perm = mf_assign_unit_blocks(own, extra, iters, simd_w);
  }
  /* pieces -> lane groups of the hosting waves, spread over those waves
   * (lane group j of each hosting wave, then j + 1) */
  for (int g = 0; g < 3; g++) {
    const int m = g < 2 ? mz : mh;
    std::vector<int> lgs;
    for (int j = 0; j < 8; j++)
      for (int w = 0; w < SAMPLE_WAVES; w++)
        if (m >> w & 1) lgs.push_back(8 * w + j);
    P.host[g].assign(NLG, -1);
    for (int p = 0; p < (int)P.pieces[g].size(); p++) P.host[g][lgs[p]] = p;
  }
  for (int w = 0; w < SAMPLE_WAVES; w++) {
    int kz = 0, kh = 0, fz = 0, fh = 0;
    for (int j = 0; j < 8; j++) {
      const int lg = 8 * w + j, ub = P.perm[lg];
      kz = std::max(kz, (int)std::max(own[ub].size(), own[NUB + ub].size()));
      kh = std::max(kh, (int)own[2 * NUB + ub].size());
      for (int g = 0; g < 3; g++)
        if (P.host[g][lg] >= 0) {
          const MfPiece &pc = P.pieces[g][P.host[g][lg]];
          (g < 2 ? fz : fh) = std::max(g < 2 ? fz : fh, pc.t1 - pc.t0);
        }
    }
    P.nzr[w] = (kz + 3) / 4;
    P.nh[w] = (kh + 3) / 4;
    P.nfzr[w] = (fz + 3) / 4;
    P.nfh[w] = (fh + 3) / 4;
    if (4 * (P.nzr[w] + P.nfzr[w]) > MF_ZMAX || 4 * (P.nh[w] + P.nfh[w]) > MF_HMAX) return -1;
  }
  return best;
}

}  // namespace

/* mfw_kernel's split form (trained Sparsify masks on the wide kernel): the
 * six R waves keep the unit blocks of `perm` (the batch's main plan, so the
 * E waves' lane-ordered tables stay valid) up to the full register caps
 * (16 z/r, 32 h blocks: the unsplit kernel's largest tables), and every
 * block beyond goes, in pieces of at most those caps, to the 16 lane groups
 * of two host waves (MFW_H_WAVES): one piece per host lane group and gate,
 * longest pieces first, dealt alternately to the two waves.  A host lane's
 * int32 partial sums reach its row's owner through LDS adds into a compact
 * part area: per gate, the unit blocks with pieces (at most 16) take part
 * rows 8 slot .. 8 slot + 7.  Exact int32 sums in any order: bit-identical
 * to the unsplit product.  Tables: [MFW_TAB_WAVES][MF_LANE_U32][64] as the
 * mf tables (host waves: their piece at slot 0 of each gate), frow
 * [3][SAMPLE_THREADS + 128]: an E thread's part row | 1 << 16 when its unit
 * has pieces (else MFW_NOROW), a host lane's target part row (else
 * MFW_NOROW).  False when a gate needs more than 16 pieces. */
bool mfw_split_tables(const std::vector<std::vector<int>> &ga, const std::vector<int> &ga_first, const int8_t *wa,
                      const MfPlanParams &pp, MfwSplitTab &T)
{
  constexpr int NUB = NA / 8, NHL = 8 * MFW_H_WAVES, FS = SAMPLE_THREADS + 64 * MFW_H_WAVES;
  const int cap[3] = {MF_ZMAX, MF_ZMAX, MF_HMAX};
  std::vector<MfPiece> pcs[3];
  std::vector<int> host[3]; /* host lane group (0..15) -> piece index */
  std::vector<int> slot_of_ub[3];
  for (int g = 0; g < 3; g++) {
    for (int u = 0; u < NUB; u++) {
      const int K = (int)ga[g * NUB + u].size();
      for (int t0 = cap[g]; t0 < K; t0 += cap[g]) pcs[g].push_back(MfPiece{u, t0, std::min(K, t0 + cap[g])});
    }
    if ((int)pcs[g].size() > NHL) return false;
    std::stable_sort(pcs[g].begin(), pcs[g].end(), [](const MfPiece &a, const MfPiece &b) { return a.t1 - a.t0 > b.t1 - b.t0; });
    host[g].assign(NHL, -1);
    for (int k = 0; k < (int)pcs[g].size(); k++) host[g][(k % MFW_H_WAVES) * 8 + k / MFW_H_WAVES] = k;
    slot_of_ub[g].assign(NUB, -1);
    int ns = 0;
    for (const MfPiece &pc : pcs[g])
      if (slot_of_ub[g][pc.unit] < 0) slot_of_ub[g][pc.unit] = ns++;
    if (ns > 16) return false;
  }
  /* own unit blocks over the six R waves for the capped rows; the E waves'
   * lane order follows.  The R waves on SIMDs 2 / 3 share them with a
   * sampler, a host wave and an E wave, all at a higher issue priority:
   * their rows are weighted 6x (the unsplit kernel's 2.5x: skewed 8,192
   * streams 486 -> 494 M, 4x-10x alike, profiles/r06/split_simdw_8192.log) */
  const std::vector<int> perm = mf_assign_unit_blocks(mf_capped_rows(ga, cap), nullptr, 40000, pp.simd_w_set ? pp.simd_w : 60);
  T.units.assign(SAMPLE_THREADS, 0);
  for (int t = 0; t < SAMPLE_THREADS; t++) T.units[t] = 8 * perm[t / 8] + (t & 7);
  T.tab.assign((size_t)MFW_TAB_WAVES * MF_LANE_U32 * 64, 0);
  T.frow.assign((size_t)3 * FS, MFW_NOROW);
  for (int w = 0; w < MFW_TAB_WAVES; w++) {
    const bool hw = w >= SAMPLE_WAVES;
    /* this wave's rows per lane group and gate */
    MfRowSpan span[3][8];
    int kz = 1, kh = 1; /* at least one slot group (zero weights: exact) */
    for (int j = 0; j < 8; j++)
      for (int g = 0; g < 3; g++) {
        MfRowSpan &s = span[g][j];
        if (!hw) {
          s.rb = g * NUB + perm[w * 8 + j];
          s.t1 = std::min((int)ga[s.rb].size(), cap[g]);
        } else if (host[g][(w - SAMPLE_WAVES) * 8 + j] >= 0) {
          const MfPiece &pc = pcs[g][host[g][(w - SAMPLE_WAVES) * 8 + j]];
          s = MfRowSpan{g * NUB + pc.unit, pc.t0, pc.t1};
          for (int r = 0; r < 8; r++)
            T.frow[(size_t)g * FS + SAMPLE_THREADS + (w - SAMPLE_WAVES) * 64 + 8 * j + r] = 8 * slot_of_ub[g][pc.unit] + r;
        }
        (g < 2 ? kz : kh) = std::max(g < 2 ? kz : kh, s.t1 - s.t0);
      }
    T.nzr[w] = (kz + 3) / 4;
    T.nh[w] = (kh + 3) / 4;
    for (int g = 0; g < 3; g++)
      for (int half = 0; half < 2; half++)
        mf_fill_half_wave(ga, ga_first, wa, &span[g][4 * half], half, mf_gate_base(g), 4 * (g < 2 ? T.nzr[w] : T.nh[w]),
                          &T.tab[(size_t)w * MF_LANE_U32 * 64]);
  }
  /* the E threads' merge entries: thread t owns unit 8 perm[t / 8] + t % 8 */
  for (int g = 0; g < 3; g++)
    for (int t = 0; t < SAMPLE_THREADS; t++) {
      const int u = perm[t / 8], sl = slot_of_ub[g][u];
      if (sl >= 0) T.frow[(size_t)g * FS + t] = (8 * sl + (t % 8)) | 1 << 16;
    }
  return true;
}

/* cls: the kernel the plan serves.  1: mf_kernel at 4 streams per
 * workgroup (1024-2047 streams), whose Y -> X half is bound by the GRU_A
 * recurrent product of the waves sharing a SIMD with a sampler (~3x the
 * cycles per MFMA of a wave pair): those SIMDs weighted 3.3x and a longer
 * search (same box, 1024 streams: -0.6 to -1.1 % frame step).  2:
 * mf2_kernel (from 2048 streams), whose samplers idle half of each phase:
 * 2.0x (2048 streams -2.1 %, 8192 -0.7 %).  3: mfw_kernel (its R waves
 * on SIMDs 2/3 share them with a sampler and an E wave): 2.5x (8192 and
 * 24,576 streams -1.0 / -0.8 % against 2.0x; 1.0, 1.4, 1.7, 2.3, 2.8, 3.3x
 * measured, profiles/r05/simdw_ab*.log).  0: 2.7x, one and two streams per
 * workgroup.  Split plans: 3.3x on mf_kernel<4>, 2.7x otherwise. */
bool mf_plan(const std::vector<std::vector<int>> &ga, MfPlan &P, const MfPlanParams &pp, int cls, int cls_split)
{
  if (cls_split < 0) cls_split = cls;
  const bool S4 = cls == 1;
  const int w_unsplit = cls == 1 ? 33 : cls == 2 ? 20 : cls == 3 ? 25 : MF_SAMPLER_SIMD_WEIGHT;
  constexpr int NUB = NA / 8;
  int kmax[3] = {0, 0, 0};
  for (int g = 0; g < 3; g++)
    for (int u = 0; u < NUB; u++) kmax[g] = std::max(kmax[g], (int)ga[g * NUB + u].size());
  const bool force = pp.force_split;
  if (std::max(kmax[0], kmax[1]) <= MF_ZMAX && kmax[2] <= MF_HMAX && !force) {
    P.split = false;
    const int T[3] = {MF_ZMAX, MF_ZMAX, MF_HMAX}, F[3] = {0, 0, 0};
    return mf_layout(ga, P, T, F, S4 ? 400000 : 40000, w_unsplit, pp) >= 0;
  }
  /* split plans weight the sampler SIMDs 3.3x on mf_kernel (1-4 streams per
   * workgroup: measured best plans at 256 and 1024 streams) and 2.0x on
   * mf2_kernel (skewed model, 8192 / 2048 streams -3.3 / -1.2 % against
   * 2.7x; 1.5, 1.7, 2.2, 2.4, 3.3x measured, profiles/r05/simdw_skew*.log) */
  const int w_split = cls_split == 2 ? 20 : 33;
  /* split: every own cap / piece size pair, screened with a short
   * assignment search, the best re-laid-out in full (force_split: split
   * even a model that fits -- pieces required -- for tests) */
  P.split = true;
  long best = -1;
  int bt[3] = {0, 0, 0}, bf[3] = {0, 0, 0};
  if (pp.caps_set) {
    const int *c = pp.caps;
    const int T[3] = {c[0], c[0], c[2]}, F[3] = {c[1], c[1], c[3]};
    if (mf_layout(ga, P, T, F, 40000, w_split, pp) >= 0) return true;
  }
  for (int Tz = 4; Tz <= MF_ZMAX; Tz += 4)
    for (int Fz = 0; Tz + Fz <= MF_ZMAX; Fz += 4)
      for (int Th = 4; Th <= MF_HMAX; Th += 4)
        for (int Fh = 0; Th + Fh <= MF_HMAX; Fh += 4) {
          bool need = false, fits = true;
          for (int g = 0; g < 3; g++) {
            const int T = g < 2 ? Tz : Th, F = g < 2 ? Fz : Fh;
            for (int u = 0; u < NUB; u++) {
              const int K = (int)ga[g * NUB + u].size();
              need |= K > T;
              if (K > T && F == 0) fits = false;
            }
            /* a piece size with nothing to carry is padding */
            bool any = false;
            for (int u = 0; u < NUB; u++) any |= (int)ga[g * NUB + u].size() > T;
            if (F > 0 && !any && g != 0 && g != 1) fits = false;
          }
          if (Fz > 0) {
            bool any = false;
            for (int u = 0; u < NUB; u++) any |= std::max(ga[u].size(), ga[NUB + u].size()) > (size_t)Tz;
            if (!any) fits = false;
          }
          if (!fits || (force && !need)) continue;
          MfPlan C;
          const int T[3] = {Tz, Tz, Th}, F[3] = {Fz, Fz, Fh};
          const long sc = mf_layout(ga, C, T, F, 1500, w_split, pp);
          if (sc < 0) continue;
          if (best < 0 || sc < best) {
            best = sc;
            bt[0] = bt[1] = Tz; bt[2] = Th;
            bf[0] = bf[1] = Fz; bf[2] = Fh;
          }
        }
  if (best < 0) return false; /* does not fit even split: the lockstep kernel runs it */
  return mf_layout(ga, P, bt, bf, 40000, w_split, pp) >= 0;
}

/* GRU_A: lane l of wave w = row l%8 of unit block perm[8w + l/8] of each
 * gate (units 8 perm[.] .. +7); D row of that lane = that unit.  Its own
 * region holds the first own[g] blocks of that row block; a split model's
 * hosted region [own, own + hosted) the piece of another (long) row block,
 * whose partial sums go to that row's owner */
void mf_tables(const std::vector<std::vector<int>> &ga, const std::vector<int> &ga_first, const int8_t *wa,
               const MfPlan &plan, MfTab &T)
{
  constexpr int NUB = NA / 8;
  const std::vector<int> &perm = plan.perm;
  T.tab.assign((size_t)SAMPLE_WAVES * MF_LANE_U32 * 64, 0);
  T.units.assign((size_t)SAMPLE_WAVES * 64, 0);
  T.frow.assign((size_t)3 * SAMPLE_WAVES * 64, NA); /* NA: no hosted piece (a dummy row) */
  for (int w = 0; w < SAMPLE_WAVES; w++) {
    for (int l = 0; l < 64; l++) T.units[w * 64 + l] = 8 * perm[w * 8 + (l >> 3)] + (l & 7);
    for (int g = 0; g < 3; g++) {
      const int nown = 4 * (g < 2 ? plan.nzr[w] : plan.nh[w]), nfor = 4 * (g < 2 ? plan.nfzr[w] : plan.nfh[w]);
      for (int region = 0; region < 2; region++) {
        const int nslot = region ? nfor : nown, off = region ? nown : 0;
        if (!nslot) continue;
        for (int half = 0; half < 2; half++) {
          MfRowSpan span[4];
          for (int k = 0; k < 4; k++) {
            const int lg = w * 8 + 4 * half + k;
            if (!region) {
              span[k].rb = g * NUB + perm[lg];
              span[k].t1 = std::min((int)ga[span[k].rb].size(), plan.own[g]);
            } else if (plan.host[g][lg] >= 0) {
              const MfPiece &pc = plan.pieces[g][plan.host[g][lg]];
              span[k] = MfRowSpan{g * NUB + pc.unit, pc.t0, pc.t1};
              for (int r = 0; r < 8; r++) T.frow[((size_t)g * SAMPLE_WAVES + w) * 64 + 8 * (4 * half + k) + r] = 8 * pc.unit + r;
            }
          }
          mf_fill_half_wave(ga, ga_first, wa, span, half, mf_gate_base(g) + off, nslot, &T.tab[(size_t)w * MF_LANE_U32 * 64]);
        }
      }
    }
  }
  /* bit 16 of a lane's entry of gate g: its own row (unit units[lane]) has
   * hosted pieces there, whose sums it merges after barrier X */
  for (int g = 0; g < 3; g++) {
    std::vector<char> has(NUB, 0);
    for (const MfPiece &pc : plan.pieces[g]) has[pc.unit] = 1;
    for (int t = 0; t < SAMPLE_WAVES * 64; t++)
      if (has[T.units[t] / 8]) T.frow[(size_t)g * SAMPLE_WAVES * 64 + t] |= 1 << 16;
  }
}

}  // namespace lpcnet_mi355x
