/*
 * model_host_check.cpp -- the matrix-core tables of a model load, decoded
 * back into the matrices they stand for, on the CPU.  A stand-alone program
 * over the host-only objects of the library (no device, no Python):
 *
 *   make check        (builds and runs tools/model_host_check)
 *
 *   tools/model_host_check FILE...   (the same on weight blobs; one "plan"
 *                                     line per plan on stdout: the planner's
 *                                     verdict, caps, pieces, groups per wave)
 *
 * For the int8 synthetic models (default, skewed: split plans; seed 1, then
 * the default and skewed models of seeds 2..8) in every plan
 * class (1, 512, 1024, 2048 streams; 8192 streams planned for the wide
 * kernel), and again with every plan forced to split, it decodes
 *   - mf / mf_unit / mf_frow (own and hosted regions, through the slots'
 *     column bytes) and
 *   - mfw_tab / mfw_unit / mfw_frow (R waves, host waves, part rows)
 * into a dense 1152 x 384 GRU_A recurrent matrix that must equal the one
 * assembled from the blob's index and weights: every block exactly once, at
 * its column, in a row whose partial sum reaches the right unit.  It also
 * checks the slot budgets of every wave (4 (nzr + nfzr) <= MF_ZMAX,
 * 4 (nh + nfh) <= MF_HMAX), that a lane group hosts at most one piece per
 * gate, that a gate without pieces has no merge flag and no hosted row, that
 * the wide split form exists exactly when the mask allows it, and that the
 * dense GRU_B tiles decode to the blob's GRU_B.  A model the planner
 * declines (the lockstep kernel runs it) is counted, not failed.
 *
 * For the synthetic PLC predictors (side_tables.cpp plc_parse; the default
 * shape 128 / 256 / 256 and the small one 64 / 128 / 64) it decodes the input
 * and recurrent v_mfma_i32_16x16x64_i8 A tiles of both GRUs into dense
 * [3 n][K] matrices that must equal the ones assembled from the blob's index,
 * weight and recurrent-weight records, and recomputes every seed from subias
 * and the decoded rows' sums.  The six GRUs of the synthetic RDO-VAEs
 * (rdovae_parse; the default shape and the small one) go through the same
 * check, after the dimensions derived from the record sizes.
 *
 * Under AddressSanitizer and UBSan (host code only):
 *
 *   make build_san/mf_plan.o build_san/model_host.o build_san/side_tables.o build_san/model_gen.o build_san/host_rcpps.o \
 *        BUILD=build_san EXTRA="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
 *   /opt/rocm/bin/hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Iinclude -Ilpcnet_amd/csrc \
 *        -Xarch_host -fsanitize=address,undefined -c tools/model_host_check.cpp -o build_san/model_host_check.o
 *   /opt/rocm/llvm/bin/clang++ -fsanitize=address,undefined -o build_san/model_host_check build_san/model_host_check.o \
 *        build_san/model_host.o build_san/side_tables.o build_san/mf_plan.o build_san/model_gen.o build_san/host_rcpps.o
 *   (the compiler hipcc drives: the objects' sanitizer calls need its runtime)
 *   build_san/model_host_check
 *
 * Exit status 0 and one "model_host_check ok" line when every check holds.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <vector>

#include "side_tables.h"

using namespace lpcnet_mi355x;

static int fails;

#define CHECK(cond, ...)                                    \
  do {                                                      \
    if (!(cond)) {                                          \
      if (fails++ < 20) {                                   \
        fprintf(stderr, "line %d: %s: ", __LINE__, #cond);  \
        fprintf(stderr, __VA_ARGS__);                       \
        fprintf(stderr, "\n");                              \
      }                                                     \
    }                                                       \
  } while (0)

typedef std::vector<int> Mat; /* [rows][NA] */

static int gate_base(int g) { return g == 0 ? 0 : (g == 1 ? MF_ZMAX : 2 * MF_ZMAX); }

/* slots [s0, s0 + n) of lane l of a wave's table [MF_LANE_U32][64] added into row `row` of D
 * (row < 0: the slots must hold zero weights) */
static void add_slots(const uint32_t *wtab, int l, int s0, int n, int row, Mat &D, const char *what)
{
  for (int s = s0; s < s0 + n; s++) {
    int8_t w[4];
    memcpy(w, &wtab[(size_t)s * 64 + l], 4);
    const int cb = (wtab[(size_t)(MF_GA + s / 4) * 64 + l] >> (8 * (s & 3))) & 0xFF;
    CHECK(cb < NA / 4, "%s: lane %d slot %d column block %d", what, l, s, cb);
    if (cb >= NA / 4) continue;
    for (int c = 0; c < 4; c++) {
      if (row < 0) CHECK(w[c] == 0, "%s: lane %d slot %d has weights but no row", what, l, s);
      else D[(size_t)row * NA + 4 * cb + c] += w[c];
    }
  }
}

/* slots of a lane's table outside [s0, s0 + n) of gate g's range must be zero */
static void check_unused(const uint32_t *wtab, int l, int g, int used, const char *what)
{
  const int end = gate_base(g) + (g < 2 ? MF_ZMAX : MF_HMAX);
  for (int s = gate_base(g) + used; s < end; s++)
    CHECK(wtab[(size_t)s * 64 + l] == 0, "%s: lane %d unused slot %d holds weights", what, l, s);
}

static void compare(const Mat &D, const Mat &R, const char *what, const char *tag)
{
  size_t bad = 0, first = 0;
  for (size_t i = 0; i < R.size(); i++)
    if (D[i] != R[i] && !bad++) first = i;
  CHECK(bad == 0, "%s %s: %zu entries differ, first at row %zu column %zu (%d, blob %d)", tag, what, bad, first / NA,
        first % NA, D[first], R[first]);
}

static void check_mf(const HostModel &H, const Mat &R, const char *tag)
{
  const MfTables &mt = H.sample.mf;
  Mat D(R.size(), 0);
  CHECK(H.mf.tab.size() == (size_t)SAMPLE_WAVES * MF_LANE_U32 * 64 && H.mf.units.size() == (size_t)SAMPLE_WAVES * 64 &&
            H.mf.frow.size() == (size_t)3 * SAMPLE_WAVES * 64,
        "%s: table sizes", tag);
  std::set<int> units(H.mf.units.begin(), H.mf.units.end());
  CHECK((int)units.size() == NA && *units.begin() == 0 && *units.rbegin() == NA - 1, "%s: mf_unit is not a permutation", tag);
  std::set<int> merged[3], hosted[3]; /* unit blocks whose lanes merge pieces / that pieces go to */
  for (int w = 0; w < SAMPLE_WAVES; w++) {
    CHECK(4 * (mt.mf_nzr[w] + mt.mf_nfzr[w]) <= MF_ZMAX, "%s: wave %d z/r groups %d + %d", tag, w, mt.mf_nzr[w], mt.mf_nfzr[w]);
    CHECK(4 * (mt.mf_nh[w] + mt.mf_nfh[w]) <= MF_HMAX, "%s: wave %d h groups %d + %d", tag, w, mt.mf_nh[w], mt.mf_nfh[w]);
    CHECK(H.sample.form.mf_split || (mt.mf_nfzr[w] == 0 && mt.mf_nfh[w] == 0), "%s: hosted groups in an unsplit plan", tag);
    const uint32_t *wtab = &H.mf.tab[(size_t)w * MF_LANE_U32 * 64];
    for (int l = 0; l < 64; l++) {
      const int unit = H.mf.units[w * 64 + l];
      CHECK(unit % 8 == l % 8 && unit / 8 == H.mf.units[w * 64 + (l & ~7)] / 8, "%s: lane %d of wave %d unit %d", tag, l, w, unit);
      for (int g = 0; g < 3; g++) {
        const int nown = 4 * (g < 2 ? mt.mf_nzr[w] : mt.mf_nh[w]), nfor = 4 * (g < 2 ? mt.mf_nfzr[w] : mt.mf_nfh[w]);
        const int fr = H.mf.frow[((size_t)g * SAMPLE_WAVES + w) * 64 + l], target = fr & 0xFFFF;
        if (fr >> 16) merged[g].insert(unit / 8);
        /* a gate without pieces: no lane merges, no lane hosts (z and r share their group counts, so a
         * wave can carry hosted slots of one for the other's pieces: zero weights, no row) */
        if (H.mf_pieces[g] == 0) CHECK(fr == NA, "%s: wave %d lane %d gate %d entry %#x in a gate without pieces", tag, w, l, g, fr);
        add_slots(wtab, l, gate_base(g), nown, g * NA + unit, D, tag);
        /* one piece per lane group and gate: its 8 lanes carry rows 8 u .. 8 u + 7 of one unit block u, or none */
        const int t0 = H.mf.frow[((size_t)g * SAMPLE_WAVES + w) * 64 + (l & ~7)] & 0xFFFF;
        CHECK(target == NA ? t0 == NA : (target < NA && target == t0 + l % 8 && t0 % 8 == 0), "%s: wave %d lane %d gate %d hosted row %d",
              tag, w, l, g, target);
        if (target < NA) hosted[g].insert(target / 8);
        add_slots(wtab, l, gate_base(g) + nown, nfor, target < NA ? g * NA + target : -1, D, tag);
        /* a wave with no group at all in a gate (used 0: the kernels' runtime-count default) has only
         * zero words in that gate's slots: this covers it */
        check_unused(wtab, l, g, nown + nfor, tag);
      }
    }
  }
  for (int g = 0; g < 3; g++) CHECK(merged[g] == hosted[g], "%s: gate %d merge flags do not match the hosted pieces", tag, g);
  compare(D, R, "mf tables", tag);
}

static void check_mfw(const HostModel &H, const Mat &R, const char *tag)
{
  constexpr int FS = SAMPLE_THREADS + 64 * MFW_H_WAVES;
  const MfwTables &wt = H.sample.mfw;
  const MfwSplitTab &T = H.mfw;
  Mat D(R.size(), 0);
  CHECK(T.tab.size() == (size_t)MFW_TAB_WAVES * MF_LANE_U32 * 64 && T.units.size() == (size_t)SAMPLE_THREADS &&
            T.frow.size() == (size_t)3 * FS,
        "%s: wide table sizes", tag);
  std::set<int> units(T.units.begin(), T.units.end());
  CHECK((int)units.size() == NA, "%s: mfw_unit is not a permutation", tag);
  for (int g = 0; g < 3; g++) {
    /* part row -> unit, from the E threads' merge entries */
    std::vector<int> unit_of(MFW_PART_ROWS, -1);
    for (int t = 0; t < SAMPLE_THREADS; t++) {
      const int fr = T.frow[(size_t)g * FS + t];
      if (fr == MFW_NOROW) continue;
      const int pr = fr & 0xFFFF;
      CHECK(fr >> 16 == 1 && pr < MFW_PART_ROWS && pr % 8 == t % 8, "%s: gate %d thread %d entry %#x", tag, g, t, fr);
      if (pr >= MFW_PART_ROWS) continue;
      CHECK(unit_of[pr] < 0, "%s: gate %d part row %d merged twice", tag, g, pr);
      unit_of[pr] = T.units[t];
    }
    for (int w = 0; w < MFW_TAB_WAVES; w++) {
      const int n = 4 * (g < 2 ? wt.mfw_nzr[w] : wt.mfw_nh[w]);
      CHECK(n >= 4 && n <= (g < 2 ? MF_ZMAX : MF_HMAX), "%s: table wave %d gate %d slots %d", tag, w, g, n);
      CHECK(wt.mfw_nzr[w] == T.nzr[w] && wt.mfw_nh[w] == T.nh[w], "%s: table wave %d group counts", tag, w);
      const uint32_t *wtab = &T.tab[(size_t)w * MF_LANE_U32 * 64];
      for (int l = 0; l < 64; l++) {
        int row = -1;
        if (w < SAMPLE_WAVES) {
          row = g * NA + T.units[w * 64 + l];
        } else {
          const int pr = T.frow[(size_t)g * FS + SAMPLE_THREADS + (w - SAMPLE_WAVES) * 64 + l];
          const int p0 = T.frow[(size_t)g * FS + SAMPLE_THREADS + (w - SAMPLE_WAVES) * 64 + (l & ~7)];
          CHECK(pr == MFW_NOROW ? p0 == MFW_NOROW : (pr < MFW_PART_ROWS && p0 % 8 == 0 && pr == p0 + l % 8),
                "%s: host wave %d lane %d gate %d part row %d", tag, w, l, g, pr);
          if (pr != MFW_NOROW && pr < MFW_PART_ROWS) {
            CHECK(unit_of[pr] >= 0, "%s: gate %d part row %d has no owner", tag, g, pr);
            if (unit_of[pr] >= 0) row = g * NA + unit_of[pr];
          }
        }
        add_slots(wtab, l, gate_base(g), n, row, D, tag);
        check_unused(wtab, l, g, n, tag);
      }
    }
  }
  compare(D, R, "wide split tables", tag);
}

/* the dense GRU_B tiles against the blob's GRU_B (input: block-sparse; recurrent: [rb][cb][8][4]) */
static void check_gru_b(const HostModel &H, const char *tag)
{
  std::vector<std::vector<int>> gb;
  const Arr *w = find(H.records, "gru_b_weights"), *r = find(H.records, "gru_b_recurrent_weights");
  if (!parse_idx(H.records, "gru_b_weights_idx", NA, GB_ROWS, gb) || !w || !r) {
    CHECK(false, "%s: GRU_B records", tag);
    return;
  }
  std::vector<int> Rin((size_t)GB_ROWS * NA, 0), Rrec((size_t)GB_ROWS * NB, 0), Din(Rin.size(), 0), Drec(Rrec.size(), 0);
  const int8_t *wb = (const int8_t *)w->data, *wr = (const int8_t *)r->data;
  int k = 0;
  for (int rb = 0; rb < GB_ROWS / 8; rb++)
    for (int pos : gb[rb]) {
      for (int i = 0; i < 8; i++)
        for (int c = 0; c < 4; c++) Rin[(size_t)(rb * 8 + i) * NA + pos + c] += wb[32 * k + 4 * i + c];
      k++;
    }
  for (int rb = 0; rb < GB_ROWS / 8; rb++)
    for (int cb = 0; cb < NB / 4; cb++)
      for (int i = 0; i < 8; i++)
        for (int c = 0; c < 4; c++) Rrec[(rb * 8 + i) * NB + 4 * cb + c] = wr[32 * (rb * (NB / 4) + cb) + 4 * i + c];
  CHECK(H.mf_gb.size() == (size_t)MF_GB_TILES * 64 * 4, "%s: GRU_B tile size", tag);
  if (H.mf_gb.size() != (size_t)MF_GB_TILES * 64 * 4) return;
  const int8_t *tiles = (const int8_t *)H.mf_gb.data();
  for (int g = 0; g < 3; g++)
    for (int l = 0; l < 64; l++) {
      const int row = 16 * g + (l & 15), k0 = 16 * (l >> 4);
      for (int kt = 0; kt < 6; kt++)
        for (int j = 0; j < 16; j++) Din[(size_t)row * NA + 64 * kt + k0 + j] += tiles[((size_t)(g * 6 + kt) * 64 + l) * 16 + j];
      for (int j = 0; j < 16; j++) {
        const int v = tiles[((size_t)(MF_GB_IN + g) * 64 + l) * 16 + j];
        if (k0 == 0) Drec[row * NB + j] += v;
        else CHECK(v == 0, "%s: recurrent tile %d lane %d byte %d", tag, g, l, j);
      }
    }
  CHECK(Din == Rin, "%s: GRU_B input tiles differ from the blob", tag);
  CHECK(Drec == Rrec, "%s: GRU_B recurrent tiles differ from the blob", tag);
}

/* mfw_kernel's split form, from the mask alone: it exists exactly when every
 * gate's blocks beyond the register caps (MF_ZMAX / MF_ZMAX / MF_HMAX per
 * row) make at most 16 pieces of at most a cap each (one per lane group of
 * the two host waves) over at most 16 unit blocks (the part area's rows) */
static bool wide_split_exists(const GruASparse &A)
{
  constexpr int NUB = NA / 8;
  for (int g = 0; g < 3; g++) {
    const int cap = g < 2 ? MF_ZMAX : MF_HMAX;
    int pieces = 0, units = 0;
    for (int u = 0; u < NUB; u++) {
      const int beyond = (int)A.blocks[g * NUB + u].size() - cap;
      if (beyond <= 0) continue;
      pieces += (beyond + cap - 1) / cap;
      units++;
    }
    if (pieces > 8 * MFW_H_WAVES || units > MFW_PART_ROWS / 8) return false;
  }
  return true;
}

static int plans, split_plans, wide_plans, declined;

/* One blob in every plan class, as planned and with every plan forced to
 * split.  mf: 1 / 0 = the planner must take / decline the model, -1 = either
 * (a declined plan is counted, the lockstep kernel runs such a model).
 * report: one "plan" line per plan on stdout. */
static void check_model(const char *name, const unsigned char *blob, int n, int mf, bool report)
{
  static const struct { int streams; bool wide; } classes[] = {{1, false}, {512, false}, {1024, false}, {2048, false}, {8192, true}};
  /* the matrix the tables must decode to */
  std::vector<Arr> L;
  GruASparse A;
  if (!parse_blob(L, blob, n) || parse_gru_a(L, A)) {
    CHECK(false, "%s: blob does not parse (%s)", name, last_err().c_str());
    return;
  }
  const bool int8 = A.variant == LPCNET_VARIANT_INT8;
  Mat R;
  if (int8) {
    R.assign((size_t)GA_ROWS * NA, 0);
    for (int rb = 0; rb < GA_ROWS / 8; rb++)
      for (int t = 0; t < (int)A.blocks[rb].size(); t++)
        for (int r = 0; r < 8; r++)
          for (int c = 0; c < 4; c++)
            R[(size_t)(rb * 8 + r) * NA + A.blocks[rb][t] + c] += ((const int8_t *)A.w)[32 * (A.first[rb] + t) + 4 * r + c];
  }
  for (int force = 0; force < 2; force++) {
    if (force) setenv("LPCNET_MF_FORCE_SPLIT", "1", 1);
    else unsetenv("LPCNET_MF_FORCE_SPLIT");
    for (const auto &c : classes) {
      char tag[300];
      snprintf(tag, sizeof tag, "%s/%d%s%s", name, c.streams, c.wide ? "/wide" : "", force ? "/forced split" : "");
      ModelBuildOpts opts;
      opts.streams = c.streams;
      opts.wide = c.wide;
      HostModel H;
      if (build_host_model(blob, n, opts, H)) {
        CHECK(false, "%s: build failed: %s", tag, last_err().c_str());
        continue;
      }
      const SampleForm &form = H.sample.form;
      const MfTables &mt = H.sample.mf;
      if (report) {
        printf("plan %s: variant %d may_saturate %d mf_ok %d fp_ok %d fp_long %d lockstep_streams %d", tag, H.variant, H.sat, H.mf_ok,
               H.fp_ok, H.fp_long, H.S);
        if (H.mf_ok) {
          printf(" split %d wide_split %d own %d %d %d pieces %d %d %d groups", form.mf_split, form.mfw_split, H.mf_own[0], H.mf_own[1],
                 H.mf_own[2], H.mf_pieces[0], H.mf_pieces[1], H.mf_pieces[2]);
          for (int w = 0; w < SAMPLE_WAVES; w++) printf(" (%d %d %d %d)", mt.mf_nzr[w], mt.mf_nfzr[w], mt.mf_nh[w], mt.mf_nfh[w]);
        }
        printf("\n");
      }
      CHECK(int8 || !H.mf_ok, "%s: matrix-core tables of an fp32 model", tag);
      if (mf >= 0) CHECK(H.mf_ok == (mf != 0), "%s: matrix-core tables %d", tag, H.mf_ok);
      if (!H.mf_ok) {
        declined++;
        continue;
      }
      CHECK(!force || form.mf_split, "%s: plan not split", tag);
      CHECK(form.mfw_split == (form.mf_split && c.wide && wide_split_exists(A) ? 1 : 0), "%s: wide split form %d", tag, form.mfw_split);
      check_mf(H, R, tag);
      if (form.mfw_split) check_mfw(H, R, tag);
      check_gru_b(H, tag);
      plans++;
      split_plans += form.mf_split;
      wide_plans += form.mfw_split;
    }
  }
  unsetenv("LPCNET_MF_FORCE_SPLIT");
}

static int plc_decoded;

/* A tiles [unit tile][gate][k tile][64 lanes] of 16 bytes (lpcnet_engine.h PlcArgs) -> dense [3 n][K] */
static bool decode_plc_tiles(const std::vector<uint4> &tiles, int n, int K, std::vector<int> &D, const char *what)
{
  const int nk = K / 64;
  D.assign((size_t)3 * n * K, 0);
  CHECK(tiles.size() == (size_t)(n / 16) * 3 * nk * 64, "%s: %zu tiles for n %d K %d", what, tiles.size(), n, K);
  if (tiles.size() != (size_t)(n / 16) * 3 * nk * 64) return false;
  const int8_t *by = (const int8_t *)tiles.data();
  for (int ut = 0; ut < n / 16; ut++)
    for (int g = 0; g < 3; g++)
      for (int kt = 0; kt < nk; kt++)
        for (int l = 0; l < 64; l++) {
          const int row = g * n + 16 * ut + l % 16, k0 = 64 * kt + 16 * (l / 16);
          for (int j = 0; j < 16; j++) D[(size_t)row * K + k0 + j] += by[((((size_t)ut * 3 + g) * nk + kt) * 64 + l) * 16 + j];
        }
  return true;
}

/* One compute_gruB layer `nm` of nin inputs and n units: its input and
 * recurrent A tiles decode to the matrices assembled from the blob's
 * _weights_idx / _weights / _recurrent_weights records (as check_gru_b
 * assembles GRU_B's), and every seed is rne(subias * 128 * 127) + 128 * the
 * decoded row's sum. */
static bool check_gru_tiles(const std::vector<Arr> &L, const char *name, const std::string &nm, int nin, int n,
                            const std::vector<uint4> &g_in, const std::vector<uint4> &g_rec, const std::vector<int> &seed)
{
  char tag[80];
  snprintf(tag, sizeof tag, "%s/%s", name, nm.c_str());
  std::vector<std::vector<int>> blocks;
  const Arr *w = find(L, (nm + "_weights").c_str()), *r = find(L, (nm + "_recurrent_weights").c_str());
  const Arr *sb = find(L, (nm + "_subias").c_str());
  if (!parse_idx(L, (nm + "_weights_idx").c_str(), nin, 3 * n, blocks) || !w || !r || !sb || sb->size != 24 * n ||
      w->size != 32 * total_blocks(blocks) || r->size != 3 * n * n) {
    CHECK(false, "%s: records", tag);
    return false;
  }
  std::vector<int> Rin((size_t)3 * n * nin, 0), Rrec((size_t)3 * n * n, 0), Din, Drec;
  const int8_t *wb = (const int8_t *)w->data, *wr = (const int8_t *)r->data;
  int t = 0;
  for (int rb = 0; rb < 3 * n / 8; rb++)
    for (int pos : blocks[rb]) {
      for (int i = 0; i < 8; i++)
        for (int c = 0; c < 4; c++) Rin[(size_t)(rb * 8 + i) * nin + pos + c] += wb[32 * t + 4 * i + c];
      t++;
    }
  for (int rb = 0; rb < 3 * n / 8; rb++)
    for (int cb = 0; cb < n / 4; cb++)
      for (int i = 0; i < 8; i++)
        for (int c = 0; c < 4; c++) Rrec[(size_t)(rb * 8 + i) * n + 4 * cb + c] = wr[32 * ((size_t)rb * (n / 4) + cb) + 4 * i + c];
  if (!decode_plc_tiles(g_in, n, nin, Din, tag) || !decode_plc_tiles(g_rec, n, n, Drec, tag)) return false;
  CHECK(Din == Rin, "%s: input tiles differ from the blob", tag);
  CHECK(Drec == Rrec, "%s: recurrent tiles differ from the blob", tag);
  CHECK(seed.size() == (size_t)6 * n, "%s: %zu seeds", tag, seed.size());
  if (seed.size() != (size_t)6 * n) return false;
  const float *subias = (const float *)sb->data;
  for (int half = 0; half < 2; half++) {
    const std::vector<int> &D = half ? Drec : Din;
    const int K = half ? n : nin;
    for (int row = 0; row < 3 * n; row++) {
      int sum = 0;
      for (int j = 0; j < K; j++) sum += D[(size_t)row * K + j];
      /* _mm256_cvtps_epi32: round to nearest even; the synthetic subias stay far inside the int range */
      const float v = subias[half * 3 * n + row] * (128.f * 127.f);
      CHECK(fabsf(v) < 2147483648.f, "%s: subias %d of half %d out of range", tag, row, half);
      if (!(fabsf(v) < 2147483648.f)) continue;
      const int want = (int)((uint32_t)(int)nearbyintf(v) + (uint32_t)(128 * sum));
      CHECK(seed[half * 3 * n + row] == want, "%s: seed %d of half %d is %d, recomputed %d", tag, row, half,
            seed[half * 3 * n + row], want);
    }
  }
  return true;
}

/* The PLC predictor of a synthetic blob: both GRUs under check_gru_tiles. */
static void check_plc(const char *name, int flags, int cond, int n1, int n2)
{
  const int len = lpcnet_mi355x_synthetic_model(1, LPCNET_VARIANT_INT8, flags, nullptr, 0);
  std::vector<unsigned char> blob(len);
  lpcnet_mi355x_synthetic_model(1, LPCNET_VARIANT_INT8, flags, blob.data(), len);
  std::vector<Arr> L;
  PlcHost P;
  if (!parse_blob(L, blob.data(), len) || plc_parse(L, LPCNET_VARIANT_INT8, P, true)) {
    CHECK(false, "%s: PLC records do not parse (%s)", name, last_err().c_str());
    return;
  }
  CHECK(P.cond == cond && P.n[0] == n1 && P.n[1] == n2, "%s: dims %d %d %d", name, P.cond, P.n[0], P.n[1]);
  int nin = P.cond;
  for (int k = 0; k < 2; k++) {
    if (!check_gru_tiles(L, name, k ? "plc_gru2" : "plc_gru1", nin, P.n[k], P.g_in[k], P.g_rec[k], P.seed[k])) return;
    nin = P.n[k];
  }
  plc_decoded++;
}

static int rdovae_decoded;

/* The RDO-VAE of a synthetic blob: the dimensions from the record sizes and
 * the six GRUs under check_gru_tiles. */
static void check_rdovae(const char *name, int flags, int T, int lat, int sd, int g1)
{
  const int len = lpcnet_mi355x_synthetic_model(1, LPCNET_VARIANT_INT8, flags, nullptr, 0);
  std::vector<unsigned char> blob(len);
  lpcnet_mi355x_synthetic_model(1, LPCNET_VARIANT_INT8, flags, blob.data(), len);
  std::vector<Arr> L;
  RdovaeHost R;
  if (!parse_blob(L, blob.data(), len) || rdovae_parse(L, LPCNET_VARIANT_INT8, R, true) || !R.enc.ok || !R.dec.ok) {
    CHECK(false, "%s: RDO-VAE records do not parse (%s)", name, last_err().c_str());
    return;
  }
  int dims[RDOVAE_DIMS];
  rdovae_dims_of(R, dims);
  CHECK(dims[0] == lat && dims[1] == sd && dims[2] == T && dims[3] == 4 && dims[12] == g1, "%s: encoder dims %d %d %d %d %d", name,
        dims[0], dims[1], dims[2], dims[3], dims[12]);
  CHECK(dims[13] == lat && dims[14] == sd && dims[15] == T, "%s: decoder dims %d %d %d", name, dims[13], dims[14], dims[15]);
  for (int dec = 0; dec < 2; dec++) {
    const RdovaeSide &S = dec ? R.dec : R.enc;
    for (int k = 0; k < 3; k++) {
      const RdovaeGruHost &G = S.g[k];
      const std::string nm = std::string(dec ? "dec_dense" : "enc_dense") + std::to_string(2 * k + 2);
      CHECK(G.in == S.width[2 * k] && G.n == S.width[2 * k + 1], "%s/%s: %d -> %d", name, nm.c_str(), G.in, G.n);
      if (!check_gru_tiles(L, name, nm, G.in, G.n, G.win, G.wrec, G.seed)) return;
    }
  }
  rdovae_decoded++;
}

static bool read_file(const char *path, std::vector<unsigned char> &out)
{
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  unsigned char buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
  fclose(f);
  return true;
}

/* model_host_check            the synthetic int8 models of seed 1 (default, saturating, skewed), then the default and
 *                             skewed models of seeds 2..8
 * model_host_check FILE...    the given blobs, with one "plan" line per plan class on stdout */
int main(int argc, char **argv)
{
  static const char *const hooks[] = {"LPCNET_MF_ITERS", "LPCNET_MF_SIMD_W", "LPCNET_MF_HOSTED_F", "LPCNET_MF_PIECE_W",
                                      "LPCNET_MF_CAPS", "LPCNET_MF_FORCE_SPLIT", "LPCNET_NO_MFMA", "LPCNET_NO_MFW_SPLIT",
                                      "LPCNET_RCP", "LPCNET_VERBOSE"};
  for (const char *h : hooks) unsetenv(h);
  for (int i = 1; i < argc; i++) {
    std::vector<unsigned char> blob;
    if (!read_file(argv[i], blob)) {
      CHECK(false, "%s: cannot read", argv[i]);
      continue;
    }
    check_model(argv[i], blob.data(), (int)blob.size(), -1, true);
  }
  if (argc < 2) {
    /* a skewed model of another seed may or may not fit the register tables split: either is right */
    static const struct { const char *name; int flags; int mf, mf_other_seeds; } models[] = {
        {"int8", 0, 1, 1}, {"int8_saturating", 1, 0, -2}, {"int8_skewed", 2, 1, -1}};
    for (unsigned seed = 1; seed <= 8; seed++)
      for (const auto &m : models) {
        if (seed > 1 && m.mf_other_seeds < -1) continue;
        const int n = lpcnet_mi355x_synthetic_model(seed, LPCNET_VARIANT_INT8, m.flags, nullptr, 0);
        std::vector<unsigned char> blob(n);
        lpcnet_mi355x_synthetic_model(seed, LPCNET_VARIANT_INT8, m.flags, blob.data(), n);
        char name[64];
        snprintf(name, sizeof name, "%s/seed %u", m.name, seed);
        check_model(name, blob.data(), n, seed == 1 ? m.mf : m.mf_other_seeds, false);
      }
    /* synthetic-model flags 8: PLC records in the default shape, 8 | 16: in the small one */
    check_plc("plc", 8, 128, 256, 256);
    check_plc("plc_small", 8 | 16, 64, 128, 64);
    /* flags 32: RDO-VAE records in the default shape, 32 | 64: in the small one */
    check_rdovae("rdovae", 32, 2048, 80, 24, 128);
    check_rdovae("rdovae_small", 32 | 64, 704, 40, 32, 64);
  }
  if (fails) {
    fprintf(stderr, "model_host_check: %d checks failed\n", fails);
    return 1;
  }
  printf("model_host_check ok (%d plans decoded, %d split, %d with the wide split form; %d declined by the planner; "
         "%d PLC predictors and %d RDO-VAEs decoded)\n",
         plans, split_plans, wide_plans, declined, plc_decoded, rdovae_decoded);
  return 0;
}
