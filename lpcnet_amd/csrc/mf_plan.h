/*
 * mf_plan.h -- the GRU_A work plan of the matrix-core kernels (mf_kernel,
 * mf2_kernel, mfw_kernel) and the per-lane register tables built from it.
 * Host arithmetic on the blob's block index and int8 weights only: no device
 * call, no global state; the tuning hooks arrive as one MfPlanParams value.
 */
#ifndef LPCNET_MF_PLAN_H
#define LPCNET_MF_PLAN_H

#include <stdint.h>

#include <vector>

#include "lpcnet_engine.h"

namespace lpcnet_mi355x {

#ifndef MF_SAMPLER_SIMD_WEIGHT
#define MF_SAMPLER_SIMD_WEIGHT 27
#endif
#ifndef MF_HOSTED_WEIGHT
#define MF_HOSTED_WEIGHT 14 /* tenths: cost of a hosted slot relative to an own one */
#endif
#ifndef MF_PIECE_WEIGHT
#define MF_PIECE_WEIGHT 10 /* tenths of a score unit per hosted piece (its LDS atomics) */
#endif
#ifndef MF_HOST_ADD_SLOTS
#define MF_HOST_ADD_SLOTS 4
#endif

/* The planner's tuning hooks, read once (mf_plan_params_from_env) and passed
 * down.  simd_w (LPCNET_MF_SIMD_W) replaces the sampler-SIMD weight of every
 * search, the per-class weights of mf_plan and the 60 of mfw_split_tables
 * alike; iters (LPCNET_MF_ITERS) the iteration count of every layout's
 * assignment search (not of mfw_split_tables' own); caps (LPCNET_MF_CAPS
 * "Tz,Fz,Th,Fh": own caps and piece sizes in blocks) is tried before the
 * split search; force_split (LPCNET_MF_FORCE_SPLIT) splits even a model that
 * fits -- pieces required -- for tests. */
struct MfPlanParams {
  bool simd_w_set = false, iters_set = false, caps_set = false, force_split = false;
  int simd_w = MF_SAMPLER_SIMD_WEIGHT;
  int iters = 0;
  int hosted_f = MF_HOSTED_WEIGHT; /* LPCNET_MF_HOSTED_F */
  int piece_w = MF_PIECE_WEIGHT;   /* LPCNET_MF_PIECE_W */
  int caps[4] = {0, 0, 0, 0};
};
MfPlanParams mf_plan_params_from_env();

/* mf_kernel work plan of the GRU_A recurrent product.
 *
 * Each GRU_A lane group (8 lanes) owns one unit block (8 units, one 8-row
 * block row per gate) and runs, per gate, `own` slots of its row's blocks.
 * A trained model's block rows can be far longer than the mean -- Sparsify
 * keeps blocks by a global per-gate energy threshold (training_tf2/
 * lpcnet.py:140-160) -- so a row longer than the own cap is split: its first
 * own[g] blocks stay with the owner, the rest go in pieces of at most
 * piece[g] blocks to other lane groups' hosted region (at most one piece per
 * lane group and gate), whose int32 partial sums the kernel adds into the
 * owner's accumulator through LDS.  Integer sums are exact in any order, so
 * the result is bit-identical to the unsplit product. */
struct MfPiece {
  int unit, t0, t1; /* blocks [t0, t1) of unit block `unit`'s row of the gate */
};
struct MfPlan {
  bool split = false;
  std::vector<int> perm;               /* lane group -> own unit block */
  int own[3] = {MF_ZMAX, MF_ZMAX, MF_HMAX};
  std::vector<MfPiece> pieces[3];
  std::vector<int> host[3];            /* lane group -> piece index (-1 none) */
  int nzr[SAMPLE_WAVES] = {}, nh[SAMPLE_WAVES] = {}, nfzr[SAMPLE_WAVES] = {}, nfh[SAMPLE_WAVES] = {};
};

/* ga: the blob's GRU_A block index, [3 NA / 8] block rows of input offsets.
 * cls: the kernel the plan serves (see mf_plan.cpp); cls_split: the class of
 * a split plan's weights (default cls).  False: the model does not fit the
 * register tables even split. */
bool mf_plan(const std::vector<std::vector<int>> &ga, MfPlan &P, const MfPlanParams &pp, int cls = 0, int cls_split = -1);

/* The plan's register tables: tab [SAMPLE_WAVES][MF_LANE_U32][64] (see
 * lpcnet_engine.h MF_ZMAX), units [SAMPLE_WAVES * 64] the GRU_A unit of each
 * lane, frow [3][SAMPLE_WAVES * 64] the row each lane's hosted partial sums
 * belong to (NA: none) | 1 << 16 when the lane's own row has hosted pieces.
 * ga_first: prefix sums of the block rows' lengths; wa: the blob's int8
 * blocks (32 bytes each). */
struct MfTab {
  std::vector<uint32_t> tab;
  std::vector<int> units, frow;
};
void mf_tables(const std::vector<std::vector<int>> &ga, const std::vector<int> &ga_first, const int8_t *wa,
               const MfPlan &plan, MfTab &T);

/* mfw_kernel's split form (see mf_plan.cpp mfw_split_tables) */
struct MfwSplitTab {
  int nzr[MFW_TAB_WAVES] = {}, nh[MFW_TAB_WAVES] = {};
  std::vector<uint32_t> tab;
  std::vector<int> frow;
  std::vector<int> units; /* [SAMPLE_THREADS] own unit of each lane */
};
bool mfw_split_tables(const std::vector<std::vector<int>> &ga, const std::vector<int> &ga_first, const int8_t *wa,
                      const MfPlanParams &pp, MfwSplitTab &T);

}  // namespace lpcnet_mi355x

#endif
