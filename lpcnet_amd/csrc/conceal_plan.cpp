/*
 * conceal_plan.cpp -- lpcnet_plc_update_causal / lpcnet_plc_conceal_causal
 * (lpcnet_plc.c:188-337) and lpcnet_plc_update_non_causal /
 * lpcnet_plc_conceal_non_causal (:339-492), PLC_SKIP_UPDATES defined, as a
 * planner over the control state: see conceal_plan.h.  Host only, system
 * compiler.
 */
#include "conceal_plan.h"

#include <algorithm>
#include <map>

namespace lpcnet_mi355x {

ConcealCtrl conceal_ctrl_reset(int features_delay)
{
  ConcealCtrl c{};
  c.pcm_fill = conceal_buf_size(features_delay); /* :53; the RNN_CLEAR of :47 zeroes the rest */
  return c;
}

bool conceal_ctrl_ok(const ConcealCtrl &c, int D, int options)
{
  const int buf = conceal_buf_size(D);
  if ((options & 3) == CONCEAL_OPT_NONCAUSAL) {
    /* a queued update is set by a received tick and consumed by the next tick's first step */
    if (D != 0 || c.pcm_fill != buf || c.skip_analysis || c.blend || c.feature_buffer_fill || c.fec_read_pos || c.fec_keep_pos) return false;
    if (c.queued_update != 0 && !(c.queued_update == 1 && c.loss_count == 0)) return false;
  } else if (c.queued_update) {
    return false;
  }
  const bool fill_ok = c.pcm_fill == 0 || (c.pcm_fill >= CONCEAL_HALF && c.pcm_fill <= buf && (c.pcm_fill - CONCEAL_HALF) % CONCEAL_FRAME == 0);
  return fill_ok && c.skip_analysis >= 0 && (c.blend == 0 || c.blend == 1) && c.loss_count >= 0 && c.fec_skip >= 0 &&
         0 <= c.fec_keep_pos && c.fec_keep_pos <= c.fec_read_pos && c.fec_read_pos <= c.fec_fill_pos &&
         c.fec_fill_pos <= CONCEAL_MAX_FEC && c.feature_buffer_fill >= 0 && c.feature_buffer_fill <= CONCEAL_DEFER_DEPTH;
}

namespace {

struct Plan {
  ConcealCtrl c;
  int D;
  bool blending, dc;
  std::vector<ConcealStep> s;

  void step(int op, int a = 0, int b = 0) { s.push_back({op, a, b}); }

  /* run_frame_network_deferred (lpcnet.c:122-132) */
  void defer(int what)
  {
    step(CO_DEFER_PUSH, what, c.feature_buffer_fill);
    if (c.feature_buffer_fill < CONCEAL_DEFER_DEPTH) c.feature_buffer_fill++;
  }

  void keep_pos() { c.fec_keep_pos = std::max(0, std::max(c.fec_keep_pos, c.fec_read_pos - D - 1)); }

  /* get_fec_or_pred (:147-166) */
  bool fec_or_pred()
  {
    if (c.fec_read_pos != c.fec_fill_pos && c.fec_skip == 0) {
      step(CO_FEC_FETCH, c.fec_read_pos);
      c.fec_read_pos++;
      keep_pos();
      step(CO_PREDICT, CP_ROW_DISCARD);
      return true;
    }
    step(CO_PREDICT, CP_ZERO);
    if (c.fec_skip > 0) c.fec_skip--;
    return false;
  }

  /* lpcnet_plc_update_causal (:188-290) */
  void update()
  {
    if (dc) step(CO_DC_REMOVE);
    const bool blend_now = c.skip_analysis && c.blend;
    step(CO_BURG, blend_now && blending ? 1 : 0); /* :206 */
    if (c.skip_analysis) {
      if (c.blend) {
        if (blending) {
          step(CO_PLC_RESTORE, D);          /* :217 */
          step(CO_PREDICT, CP_BURG_ONLY);   /* :218 */
          for (int i = 0; i < D; i++) defer(CD_FEATURES); /* :219-222 */
          step(CO_IMPL, CONCEAL_HALF, CI_SPEC);    /* :223-224, :230 */
          step(CO_BLEND);                           /* :225-229 */
          step(CO_IMPL, CONCEAL_HALF, CI_PCM_PRE); /* :231 */
        } else {
          if (D > 0) step(CO_PLC_RESTORE, D - 1); /* :233 */
          step(CO_FEC_REWIND, D);                 /* :234, :168-173 */
          c.fec_read_pos = std::max(c.fec_read_pos - D, c.fec_keep_pos);
          step(CO_RESET_SIGNAL);                  /* :236 */
        }
        step(CO_PCM_MOVE, CM_TAIL_HALF); /* :242 */
        c.pcm_fill = CONCEAL_HALF;
      } else {
        step(CO_PCM_MOVE, CM_APPEND, c.pcm_fill); /* :245 */
        c.pcm_fill += CONCEAL_FRAME;
      }
    }
    step(CO_ANALYSIS); /* :251-254 */
    if (!c.blend) {
      step(CO_PREDICT, CP_FULL); /* :256-258 */
      step(CO_FEC_DISCARD);      /* :260-262 */
      if (c.fec_skip) c.fec_skip--;
      else if (c.fec_read_pos < c.fec_fill_pos) c.fec_read_pos++;
      keep_pos();
    }
    if (c.skip_analysis) {
      if (blending) defer(CD_ANALYSED); /* :267 */
      c.skip_analysis--;
    } else {
      step(CO_PCM_MOVE, CM_NEWEST); /* :271 */
      defer(CD_ANALYSED);           /* :275 */
      step(CO_PCM_MOVE, CM_SHIFT);  /* :280 */
    }
    c.loss_count = 0;
    if (dc) step(CO_DC_RESTORE);
    c.blend = 0;
  }

  /* lpcnet_plc_conceal_causal (:293-337) */
  void conceal()
  {
    for (int j = 0; j < c.feature_buffer_fill; j++) step(CO_FLUSH, j); /* :296 */
    c.feature_buffer_fill = 0;
    while (c.pcm_fill > 0) {
      const int n = std::min(c.pcm_fill, CONCEAL_FRAME);
      step(CO_PLC_PUSH); /* :305-306 */
      fec_or_pred();     /* :307 */
      step(CO_IMPL, n, CI_BUF);    /* :304, :308 */
      step(CO_PCM_MOVE, CM_SHIFT); /* :309 */
      c.pcm_fill -= n;
      c.skip_analysis++;
    }
    step(CO_PLC_PUSH);           /* :313-314 */
    step(CO_TAIL, CONCEAL_HALF); /* :315 */
    if (fec_or_pred()) c.loss_count = 0; /* :316-317 */
    else c.loss_count++;
    step(CO_ATTENUATE, c.loss_count);        /* :318-319 */
    step(CO_IMPL, CONCEAL_HALF, CI_PCM_OUT); /* :320 */
    step(CO_ANALYSIS);                       /* :322-328 */
    c.blend = 1;
    if (dc) step(CO_DC_CONCEAL); /* :330-335 */
  }

  /* process_queued_update (:342-347) */
  void queued()
  {
    if (c.queued_update) step(CO_IMPL, CONCEAL_FRAME, CI_QUEUE);
    c.queued_update = 0;
  }

  /* lpcnet_plc_update_non_causal (:349-450).  pcm_save (:373, :399) is the
   * caller's pcm as it stands until :440, so it takes no step of its own:
   * CO_REORDER reads pcm before it writes. */
  void update_noncausal()
  {
    queued();                                /* :362 */
    if (dc) step(CO_DC_REMOVE, CDC_NONCAUSAL); /* :363-372 */
    step(CO_BURG, c.loss_count > 0 ? 1 : 0); /* :375; its row with zero features at :380-382 */
    if (c.loss_count > 0) {
      step(CO_PREDICT, CP_BURG_ONLY);             /* :383 */
      step(CO_SYN_SAVE);                          /* :384 */
      step(CO_IMPL, CONCEAL_HALF, CI_BUF_OUT);    /* :385 */
      if (dc) step(CO_DC_REDO);                   /* :387-400 */
      step(CO_REVERSE);                           /* :403 */
      step(CO_RESET_SIGNAL);                      /* :404 */
      step(CO_IMPL, CONCEAL_FRAME, CI_REV);       /* :405 */
      step(CO_TAIL, CONCEAL_HALF, CT_REV);        /* :406 */
      step(CO_BLEND_BACK);                        /* :407-411 */
      step(CO_SYN_RESTORE);                       /* :414 */
      step(CO_QUEUE_FILL);                        /* :416-418 */
      c.queued_update = 1;
      step(CO_ANALYSIS, CA_BUF);                  /* :423-426 */
    }
    step(CO_ANALYSIS, CA_PCM); /* :429-432 */
    if (c.loss_count == 0) {
      step(CO_PREDICT, CP_FULL);                  /* :434-436 */
      step(CO_IMPL, CONCEAL_HALF, CI_ANALYSED);   /* :437 */
      step(CO_TAIL, CONCEAL_HALF, CT_PCM_PRE);    /* :438 */
    }
    step(CO_REORDER); /* :440-442 */
    c.loss_count = 0;
    if (dc) step(CO_DC_RESTORE, CDC_NONCAUSAL); /* :444-448 */
  }

  /* lpcnet_plc_conceal_non_causal (:452-492) */
  void conceal_noncausal()
  {
    queued();                            /* :456 */
    step(CO_PREDICT, CP_ZERO);           /* :459 */
    step(CO_ATTENUATE, c.loss_count);    /* :460-461: loss_count counts up at the end (:490) */
    if (c.loss_count == 0) {
      step(CO_PCM_MOVE, CM_HEAD_OUT);           /* :464 */
      step(CO_IMPL, CONCEAL_HALF, CI_BUF_HI);   /* :465 */
      step(CO_TAIL, CONCEAL_HALF, CT_PCM_HI);   /* :466 */
    } else {
      step(CO_IMPL, CONCEAL_HALF, CI_PCM_LO);   /* :468 */
      step(CO_TAIL, CONCEAL_HALF, CT_PCM_HI);   /* :469 */
      step(CO_PCM_MOVE, CM_HEAD_IN);            /* :471 */
      step(CO_ANALYSIS, CA_BUF);                /* :472-475 */
    }
    step(CO_PCM_MOVE, CM_TAIL_HALF); /* :477 */
    if (dc) step(CO_DC_CONCEAL, c.loss_count == 0 ? CDC_FIRST_LOSS : CDC_NONCAUSAL); /* :479-489 */
    c.loss_count++;
  }
};

}  // namespace

int plan_tick(ConcealCtrl &c, bool lost, int options, int features_delay, std::vector<ConcealStep> &out)
{
  const int mode = options & 3;
  if ((options & ~7) || mode == 3) return -1;
  if (features_delay < 0 || features_delay > CONCEAL_MAX_DELAY) return -1;
  if (mode == CONCEAL_OPT_NONCAUSAL && features_delay != 0) return -1; /* :357-361 */
  Plan p{c, features_delay, mode != CONCEAL_OPT_CODEC, (options & CONCEAL_OPT_DC_FILTER) != 0, {}};
  if (mode == CONCEAL_OPT_NONCAUSAL) {
    if (lost) p.conceal_noncausal();
    else p.update_noncausal();
  } else if (lost) {
    p.conceal();
  } else {
    p.update();
  }
  c = p.c;
  out.insert(out.end(), p.s.begin(), p.s.end());
  return 0;
}

int plan_fec_add(ConcealCtrl &c, bool null_add, int &store, int &move_from, int &move_rows)
{
  store = -1;
  move_from = move_rows = 0;
  if (null_add) {
    c.fec_skip++;
    return 0;
  }
  if (c.fec_fill_pos == CONCEAL_MAX_FEC) {
    if (c.fec_keep_pos == 0) return -1; /* "FEC buffer full" (:118-119) */
    move_from = c.fec_keep_pos;
    move_rows = c.fec_fill_pos - c.fec_keep_pos;
    c.fec_fill_pos -= c.fec_keep_pos;
    c.fec_read_pos -= c.fec_keep_pos;
    c.fec_keep_pos = 0;
  }
  store = c.fec_fill_pos++;
  return 0;
}

std::vector<ConcealGroup> merge_tick(const std::vector<std::vector<ConcealStep>> &lists, const std::vector<int> &weight)
{
  std::vector<std::vector<ConcealStep>> run(lists.size());
  for (size_t c = 0; c < lists.size(); c++)
    for (const ConcealStep &x : lists[c])
      if (x.op != CO_FEC_REWIND && x.op != CO_FEC_DISCARD) run[c].push_back(x);
  std::vector<ConcealGroup> out;
  std::vector<size_t> cur(run.size(), 0);
  for (;;) {
    std::map<ConcealStep, std::vector<int>> at; /* next step -> the classes that stand at it */
    for (size_t c = 0; c < run.size(); c++)
      if (cur[c] < run[c].size()) at[run[c][cur[c]]].push_back((int)c);
    if (at.empty()) break;
    std::vector<const std::pair<const ConcealStep, std::vector<int>> *> go;
    for (const auto &g : at) {
      bool awaited = false; /* by a class that stands elsewhere and has this step ahead of it */
      for (size_t c = 0; c < run.size() && !awaited; c++)
        if (cur[c] < run[c].size() && !(run[c][cur[c]] == g.first))
          awaited = std::find(run[c].begin() + cur[c] + 1, run[c].end(), g.first) != run[c].end();
      if (!awaited) go.push_back(&g);
    }
    if (go.empty()) {
      const auto *best = &*at.begin();
      long most = -1;
      for (const auto &g : at) {
        long n = 0;
        for (int c : g.second) n += weight[c];
        if (n > most) {
          most = n;
          best = &g;
        }
      }
      go.push_back(best);
    }
    for (const auto *g : go) {
      out.push_back({g->first, g->second});
      for (int c : g->second) cur[c]++;
    }
  }
  return out;
}

void plan_fec_clear(ConcealCtrl &c) { c.fec_keep_pos = c.fec_read_pos = c.fec_fill_pos = c.fec_skip = 0; }

}  // namespace lpcnet_mi355x
