/*
 * conceal_plan_check.cpp -- the concealment machine's planner
 * (lpcnet_amd/csrc/conceal_plan.cpp) over every loss pattern of ten ticks, on
 * the CPU.  A stand-alone program over that one host-only object:
 *
 *   make check        (builds and runs tools/conceal_plan_check)
 *
 * For each of the 1,024 patterns of lost / received ticks, in the causal and
 * the codec mode, with and without the DC filter, at FEATURES_DELAY 0..4 and
 * under three FEC schedules (none; one add before every tick; five adds
 * before every third tick, a NULL add before every fourth and a clear before
 * the seventh) it plans the ten ticks of one stream from reset and checks:
 *
 *   - a tick of an all-received history holds no synthesis step (impl, tail,
 *     flush), and a received tick in general no tail;
 *   - pcm_fill is 0 or 80 + 160 k up to PLC_BUF_SIZE,
 *     0 <= fec_keep_pos <= fec_read_pos <= fec_fill_pos <= 100,
 *     feature_buffer_fill <= 4 (conceal_ctrl_ok);
 *   - every step's parameters stay inside the buffers the kernels index with
 *     them: st->pcm offsets, plc_copy and FEC rows, deferred-buffer rows and
 *     fills, sample counts;
 *   - a lost tick ends blend = 1, a received one blend = 0 and loss_count = 0;
 *   - arguments outside the supported modes are refused with the control
 *     state and the step list untouched; a full FEC queue refuses an add.
 *
 * The same 1,024 patterns in the non-causal mode, with and without the DC
 * filter, at FEATURES_DELAY 0 (the only delay the mode has; 1..4 are refused)
 * and under the three FEC schedules:
 *
 *   - only loss_count and queued_update leave their reset values, and the FEC
 *     events move the queue's fill side alone (conceal_ctrl_ok);
 *   - a received tick after a received one is one impl of 80 and one tail of
 *     80, both teacher-forced; the speculative steps (save, reverse, clear,
 *     impl 160, tail, blend, restore, queue fill) appear together, in that
 *     order, exactly in a received tick that follows a lost one, and the next
 *     tick starts with the queued impl of 160;
 *   - loss_count counts the lost ticks since the last received one, and the
 *     attenuation sees it before the increment;
 *   - no step of the causal modes' own (plc_copy, FEC fetch, deferred push,
 *     flush, rewind, discard) appears.
 *
 * Then the merge of a batch's tick (merge_tick): streams on pseudo-random
 * loss patterns, so that many control states meet in one tick, merged tick by
 * tick.  Every class's launching steps appear in its own order, each exactly
 * once, in groups whose classes all stand at that step; the sequence is no
 * longer than the position-by-position merge's.
 *
 * Under the sanitizers:
 *
 *   mkdir -p build_san
 *   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer -Ilpcnet_amd/csrc \
 *       -o build_san/conceal_plan_check_asan tools/conceal_plan_check.cpp lpcnet_amd/csrc/conceal_plan.cpp
 *   build_san/conceal_plan_check_asan
 *
 * Exit status 0 and one "conceal_plan_check ok" line when every check holds.
 */
#include <stdio.h>
#include <string.h>

#include <vector>

#include "conceal_plan.h"

using namespace lpcnet_mi355x;

static int fails = 0;

#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (fails++ < 20) {                                  \
        fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond); \
        fprintf(stderr, __VA_ARGS__);                      \
        fprintf(stderr, "\n");                             \
      }                                                    \
    }                                                      \
  } while (0)

static const int TICKS = 10;

/* the FEC events before tick t under schedule f */
static void fec_events(ConcealCtrl &c, int f, int t)
{
  int store, from, rows;
  if (f == 1) (void)plan_fec_add(c, false, store, from, rows);
  if (f == 2) {
    if (t == 7) plan_fec_clear(c);
    if (t % 4 == 3) (void)plan_fec_add(c, true, store, from, rows);
    if (t % 3 == 0)
      for (int k = 0; k < 5; k++) (void)plan_fec_add(c, false, store, from, rows);
  }
}

static void check_step(const ConcealStep &s, bool lost, bool all_received, int D, int options, unsigned pattern)
{
  const int buf = conceal_buf_size(D), size = buf + CONCEAL_FRAME;
  const bool dc = (options & CONCEAL_OPT_DC_FILTER) != 0;
  switch (s.op) {
  case CO_DC_REMOVE:
  case CO_DC_RESTORE: CHECK(dc && !lost, "pattern %#x", pattern); break;
  case CO_DC_CONCEAL: CHECK(dc && lost, "pattern %#x", pattern); break;
  case CO_BURG: CHECK(!lost && (s.a == 0 || s.a == 1), "pattern %#x", pattern); break;
  case CO_ANALYSIS:
  case CO_BLEND:
  case CO_RESET_SIGNAL:
  case CO_FEC_DISCARD:
  case CO_PLC_PUSH: break;
  case CO_PREDICT: CHECK(s.a >= CP_FULL && s.a <= CP_ZERO, "predict %d", s.a); break;
  case CO_PLC_RESTORE: CHECK(s.a >= 0 && s.a <= D, "plc_copy[%d], delay %d", s.a, D); break;
  case CO_FEC_FETCH: CHECK(s.a >= 0 && s.a < CONCEAL_MAX_FEC, "fec[%d]", s.a); break;
  case CO_DEFER_PUSH: CHECK((s.a == CD_FEATURES || s.a == CD_ANALYSED) && s.b >= 0 && s.b <= CONCEAL_DEFER_DEPTH, "push %d fill %d", s.a, s.b); break;
  case CO_FLUSH: CHECK(lost && s.a >= 0 && s.a < CONCEAL_DEFER_DEPTH, "flush %d", s.a); break;
  case CO_IMPL:
    CHECK(s.b >= CI_BUF && s.b <= CI_PCM_OUT && (s.a == CONCEAL_HALF || (s.b == CI_BUF && s.a == CONCEAL_FRAME)), "impl(%d) kind %d", s.a, s.b);
    CHECK(lost == (s.b == CI_BUF || s.b == CI_PCM_OUT), "impl kind %d on a %s tick", s.b, lost ? "lost" : "received");
    break;
  case CO_TAIL: CHECK(lost && s.a == CONCEAL_HALF, "tail(%d)", s.a); break;
  case CO_ATTENUATE: CHECK(lost && s.a >= 0, "attenuate(%d)", s.a); break;
  case CO_PCM_MOVE:
    CHECK(s.a >= CM_TAIL_HALF && s.a <= CM_SHIFT, "move %d", s.a);
    if (s.a == CM_APPEND) CHECK(s.b >= 0 && s.b + CONCEAL_FRAME <= size, "append at %d of %d", s.b, size);
    break;
  case CO_FEC_REWIND: CHECK(s.a == D, "rewind %d", s.a); break;
  default: CHECK(false, "unknown op %d", s.op);
  }
  if (all_received) CHECK(s.op != CO_IMPL && s.op != CO_TAIL && s.op != CO_FLUSH, "pattern %#x: synthesis step %d without a loss", pattern, s.op);
}

static bool k_first_is_queue(const std::vector<ConcealStep> &s)
{
  return !s.empty() && s[0].op == CO_IMPL && s[0].a == CONCEAL_FRAME && s[0].b == CI_QUEUE;
}

/* one tick of the non-causal mode (lpcnet_plc.c:342-492) */
static void check_noncausal_tick(const std::vector<ConcealStep> &s, bool lost, bool prev_lost, bool queued_before, int loss_before, bool dc,
                                 unsigned pattern)
{
  std::vector<int> spec;
  int impl80 = 0, tail80 = 0, impl160 = 0, analyses = 0;
  for (size_t k = 0; k < s.size(); k++) {
    const ConcealStep &x = s[k];
    switch (x.op) {
    case CO_DC_REMOVE:
    case CO_DC_RESTORE: CHECK(dc && !lost && x.a == CDC_NONCAUSAL, "pattern %#x: DC step %d form %d", pattern, x.op, x.a); break;
    case CO_DC_REDO: CHECK(dc && !lost && prev_lost, "pattern %#x: DC redo", pattern); break;
    case CO_DC_CONCEAL: CHECK(dc && lost && x.a == (loss_before == 0 ? CDC_FIRST_LOSS : CDC_NONCAUSAL), "pattern %#x: DC conceal form %d", pattern, x.a); break;
    case CO_BURG: CHECK(!lost && x.a == (prev_lost ? 1 : 0), "pattern %#x: burg %d", pattern, x.a); break;
    case CO_ANALYSIS: CHECK(x.a == CA_PCM || x.a == CA_BUF, "analysis of %d", x.a); analyses++; break;
    case CO_PREDICT: CHECK(x.a == (lost ? CP_ZERO : prev_lost ? CP_BURG_ONLY : CP_FULL), "pattern %#x: predict %d", pattern, x.a); break;
    case CO_ATTENUATE: CHECK(lost && x.a == loss_before, "attenuate(%d) at loss_count %d", x.a, loss_before); break;
    case CO_IMPL:
      CHECK(x.b >= CI_QUEUE && x.b <= CI_PCM_LO, "impl kind %d", x.b);
      CHECK(x.a == ((x.b == CI_QUEUE || x.b == CI_REV) ? CONCEAL_FRAME : CONCEAL_HALF), "impl(%d) kind %d", x.a, x.b);
      if (x.b == CI_QUEUE) CHECK(k == 0 && queued_before, "pattern %#x: the queued update is not the tick's first step", pattern);
      if (x.a == CONCEAL_FRAME) impl160++;
      else impl80++;
      if (x.b == CI_REV) spec.push_back(x.op);
      break;
    case CO_TAIL:
      CHECK(x.a == CONCEAL_HALF && x.b >= CT_REV && x.b <= CT_PCM_HI, "tail(%d) kind %d", x.a, x.b);
      tail80++;
      if (x.b == CT_REV) spec.push_back(x.op);
      break;
    case CO_PCM_MOVE: CHECK(lost && (x.a == CM_TAIL_HALF || x.a == CM_HEAD_OUT || x.a == CM_HEAD_IN), "move %d", x.a); break;
    case CO_SYN_SAVE:
    case CO_REVERSE:
    case CO_RESET_SIGNAL:
    case CO_BLEND_BACK:
    case CO_SYN_RESTORE:
    case CO_QUEUE_FILL: spec.push_back(x.op); break;
    case CO_REORDER: CHECK(!lost, "reorder in a lost tick"); break;
    default: CHECK(false, "pattern %#x: step %d in the non-causal mode", pattern, x.op);
    }
  }
  const std::vector<int> want = {CO_SYN_SAVE, CO_REVERSE, CO_RESET_SIGNAL, CO_IMPL, CO_TAIL, CO_BLEND_BACK, CO_SYN_RESTORE, CO_QUEUE_FILL};
  CHECK(spec == (!lost && prev_lost ? want : std::vector<int>()), "pattern %#x: the speculative steps", pattern);
  CHECK((k_first_is_queue(s)) == queued_before, "pattern %#x: a queued update not consumed", pattern);
  if (!lost && !prev_lost) CHECK(impl80 == 1 && tail80 == 1 && impl160 == (queued_before ? 1 : 0) && analyses == 1, "pattern %#x: a received tick", pattern);
  if (!lost && prev_lost) CHECK(impl80 == 1 && tail80 == 1 && impl160 == 1 && analyses == 2, "pattern %#x: the first received tick", pattern);
  if (lost) CHECK(impl80 == 1 && tail80 == 1 && analyses == (loss_before ? 1 : 0), "pattern %#x: a lost tick", pattern);
}

int main()
{
  long plans = 0, steps = 0;
  for (int D = 0; D <= CONCEAL_MAX_DELAY; D++)
    for (int options : {0, 2, 4, 6})
      for (int f = 0; f < 3; f++)
        for (unsigned pattern = 0; pattern < (1u << TICKS); pattern++) {
          ConcealCtrl c = conceal_ctrl_reset(D);
          bool all_received = true;
          for (int t = 0; t < TICKS; t++) {
            const bool lost = (pattern >> t) & 1;
            fec_events(c, f, t);
            CHECK(conceal_ctrl_ok(c, D), "after the FEC events of tick %d, pattern %#x", t, pattern);
            all_received = all_received && !lost;
            std::vector<ConcealStep> s;
            CHECK(plan_tick(c, lost, options, D, s) == 0, "plan_tick refused a supported mode");
            CHECK(conceal_ctrl_ok(c, D), "tick %d of pattern %#x, delay %d, options %d: pcm_fill %d fec %d %d %d fill %d", t, pattern, D, options,
                  c.pcm_fill, c.fec_keep_pos, c.fec_read_pos, c.fec_fill_pos, c.feature_buffer_fill);
            CHECK(c.blend == (lost ? 1 : 0) && (lost || c.loss_count == 0), "blend %d loss_count %d", c.blend, c.loss_count);
            CHECK(!s.empty(), "an empty tick");
            for (const ConcealStep &x : s) check_step(x, lost, all_received, D, options, pattern);
            steps += (long)s.size();
          }
          plans++;
        }
  /* the non-causal mode */
  for (int options : {1, 5})
    for (int f = 0; f < 3; f++)
      for (unsigned pattern = 0; pattern < (1u << TICKS); pattern++) {
        ConcealCtrl c = conceal_ctrl_reset(0);
        bool prev_lost = false;
        for (int t = 0; t < TICKS; t++) {
          const bool lost = (pattern >> t) & 1;
          fec_events(c, f, t);
          CHECK(conceal_ctrl_ok(c, 0, options), "after the FEC events of tick %d, pattern %#x", t, pattern);
          const ConcealCtrl before = c;
          std::vector<ConcealStep> s;
          CHECK(plan_tick(c, lost, options, 0, s) == 0, "plan_tick refused the non-causal mode at delay 0");
          CHECK(conceal_ctrl_ok(c, 0, options), "tick %d of pattern %#x, options %d: loss_count %d queued_update %d", t, pattern, options,
                c.loss_count, c.queued_update);
          CHECK(c.loss_count == (lost ? before.loss_count + 1 : 0), "loss_count %d after %d", c.loss_count, before.loss_count);
          CHECK(c.queued_update == (!lost && prev_lost ? 1 : 0), "queued_update %d", c.queued_update);
          CHECK(c.fec_fill_pos == before.fec_fill_pos && c.fec_skip == before.fec_skip, "a tick moved the FEC queue");
          check_noncausal_tick(s, lost, before.loss_count > 0, before.queued_update != 0, before.loss_count, (options & CONCEAL_OPT_DC_FILTER) != 0,
                               pattern);
          prev_lost = lost;
          steps += (long)s.size();
        }
        plans++;
      }
  /* refusals leave everything as it was */
  {
    for (int D = 1; D <= CONCEAL_MAX_DELAY; D++) {
      ConcealCtrl c = conceal_ctrl_reset(D);
      const ConcealCtrl before = c;
      std::vector<ConcealStep> s;
      for (int options : {1, 5}) CHECK(plan_tick(c, false, options, D, s) == -1, "the non-causal mode accepted at delay %d", D);
      CHECK(s.empty() && !memcmp(&c, &before, sizeof(c)), "a refused plan_tick changed its arguments");
    }
  }
  {
    ConcealCtrl c = conceal_ctrl_reset(2);
    const ConcealCtrl before = c;
    std::vector<ConcealStep> s;
    for (int options : {1, 3, 5, 8, -1}) CHECK(plan_tick(c, true, options, 2, s) == -1, "options %d accepted", options);
    CHECK(plan_tick(c, true, 0, 5, s) == -1 && plan_tick(c, true, 0, -1, s) == -1, "a delay outside 0..4 accepted");
    CHECK(s.empty() && !memcmp(&c, &before, sizeof(c)), "a refused plan_tick changed its arguments");
    int store, from, rows;
    for (int k = 0; k < CONCEAL_MAX_FEC; k++) CHECK(plan_fec_add(c, false, store, from, rows) == 0 && store == k && rows == 0, "add %d", k);
    const ConcealCtrl full = c;
    CHECK(plan_fec_add(c, false, store, from, rows) == -1 && !memcmp(&c, &full, sizeof(c)), "add 101 into a full queue");
    /* with reads behind it the queue compacts instead */
    c.fec_read_pos = 10;
    c.fec_keep_pos = 7;
    CHECK(plan_fec_add(c, false, store, from, rows) == 0 && from == 7 && rows == 93 && store == 93 && c.fec_fill_pos == 94 &&
              c.fec_read_pos == 3 && c.fec_keep_pos == 0,
          "compaction: from %d rows %d store %d", from, rows, store);
  }
  /* the merge of a batch's tick */
  long merged = 0, positional = 0;
  for (int D : {0, 2, 4})
    for (int options : {0, 2, 4, 1, 5}) {
      if ((options & 3) == CONCEAL_OPT_NONCAUSAL && D != 0) continue;
      const int S = 97;
      std::vector<ConcealCtrl> ctrl(S, conceal_ctrl_reset(D));
      unsigned rnd = 12345u + D * 7 + options;
      for (int t = 0; t < 60; t++) {
        /* classes of this tick */
        std::vector<ConcealCtrl> key;
        std::vector<int> lostkey;
        std::vector<std::vector<ConcealStep>> lists;
        std::vector<int> weight;
        for (int s = 0; s < S; s++) {
          rnd = rnd * 1664525u + 1013904223u;
          const bool lost = (rnd >> 24) % 100 < (s % 3 == 0 ? 30u : 8u);
          if (((rnd >> 8) & 15) == 0) {
            int store, from, rows;
            (void)plan_fec_add(ctrl[s], false, store, from, rows);
          }
          size_t c = 0;
          while (c < key.size() && !(lostkey[c] == (int)lost && !memcmp(&key[c], &ctrl[s], sizeof(ConcealCtrl)))) c++;
          if (c == key.size()) {
            key.push_back(ctrl[s]);
            lostkey.push_back(lost);
            lists.emplace_back();
            weight.push_back(0);
            ConcealCtrl x = ctrl[s];
            CHECK(plan_tick(x, lost, options, D, lists.back()) == 0, "plan_tick");
          }
          weight[c]++;
          std::vector<ConcealStep> unused;
          (void)plan_tick(ctrl[s], lost, options, D, unused);
        }
        const std::vector<ConcealGroup> seq = merge_tick(lists, weight);
        std::vector<size_t> cur(lists.size(), 0);
        const auto skip = [&](size_t c) {
          while (cur[c] < lists[c].size() && (lists[c][cur[c]].op == CO_FEC_REWIND || lists[c][cur[c]].op == CO_FEC_DISCARD)) cur[c]++;
        };
        for (const ConcealGroup &g : seq) {
          CHECK(!g.classes.empty(), "an empty group");
          for (size_t i = 0; i < g.classes.size(); i++) {
            const size_t c = (size_t)g.classes[i];
            CHECK(i == 0 || g.classes[i - 1] < g.classes[i], "classes not ascending");
            skip(c);
            CHECK(cur[c] < lists[c].size() && lists[c][cur[c]] == g.step, "tick %d: class %zu is not at step %d", t, c, g.step.op);
            cur[c]++;
          }
        }
        size_t longest = 0;
        for (size_t c = 0; c < lists.size(); c++) {
          skip(c);
          CHECK(cur[c] == lists[c].size(), "tick %d: class %zu stops at %zu of %zu", t, c, cur[c], lists[c].size());
        }
        /* the position-by-position merge, for comparison */
        std::vector<std::vector<ConcealStep>> run(lists.size());
        for (size_t c = 0; c < lists.size(); c++)
          for (const ConcealStep &x : lists[c])
            if (x.op != CO_FEC_REWIND && x.op != CO_FEC_DISCARD) run[c].push_back(x);
        for (const auto &r : run) longest = r.size() > longest ? r.size() : longest;
        long pos = 0;
        for (size_t k = 0; k < longest; k++) {
          std::vector<ConcealStep> seen;
          for (const auto &r : run)
            if (k < r.size()) {
              bool dup = false;
              for (const ConcealStep &x : seen) dup = dup || x == r[k];
              if (!dup) seen.push_back(r[k]);
            }
          pos += (long)seen.size();
        }
        CHECK((long)seq.size() <= pos, "tick %d: %zu groups, %ld position by position", t, seq.size(), pos);
        merged += (long)seq.size();
        positional += pos;
      }
    }
  if (fails) {
    fprintf(stderr, "conceal_plan_check: %d checks failed\n", fails);
    return 1;
  }
  printf("conceal_plan_check ok: %ld plans, %ld steps; merged ticks: %ld groups (%ld position by position)\n", plans, steps, merged,
         positional);
  return 0;
}
