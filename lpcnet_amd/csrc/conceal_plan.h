/*
 * conceal_plan.h -- the control side of lpcnet_plc_update / lpcnet_plc_conceal
 * (lpcnet_plc.c:188-337 causal and codec, :339-492 non-causal, PLC_SKIP_UPDATES
 * defined) as a host-only planner.  What decides which primitive calls a tick
 * makes -- pcm_fill, skip_analysis, blend, loss_count, the FEC queue's
 * positions and the fill of the deferred feature buffer, in the non-causal
 * mode loss_count and queued_update alone -- depends on the sequence of lost
 * and received ticks and of FEC adds alone, never on signal data.  So a tick of a stream is
 * planned without reading anything back: plan_tick advances the control state
 * and returns the ordered list of steps, each one primitive call with its
 * parameters.  No HIP include, no device call; conceal_calls.cpp runs the
 * lists of a whole batch, tools/conceal_plan_check.cpp and
 * tests/test_conceal_plan.py check them.
 */
#ifndef LPCNET_CONCEAL_PLAN_H
#define LPCNET_CONCEAL_PLAN_H

#include <vector>

namespace lpcnet_mi355x {

constexpr int CONCEAL_FRAME = 160;         /* FRAME_SIZE */
constexpr int CONCEAL_HALF = 80;           /* TRAINING_OFFSET, FRAME_SIZE - TRAINING_OFFSET */
constexpr int CONCEAL_MAX_FEC = 100;       /* PLC_MAX_FEC (lpcnet_private.h:25) */
constexpr int CONCEAL_DEFER_DEPTH = 4;     /* MAX_FEATURE_BUFFER_SIZE; conv1 + conv2 kernel sizes - 2 of the model */
constexpr int CONCEAL_MAX_DELAY = 4;       /* FEATURES_DELAY 0..4, as the engine */
constexpr int CONCEAL_OPT_CAUSAL = 0;      /* LPCNET_PLC_CAUSAL */
constexpr int CONCEAL_OPT_NONCAUSAL = 1;   /* LPCNET_PLC_NONCAUSAL: FEATURES_DELAY 0 only (:357-361) */
constexpr int CONCEAL_OPT_CODEC = 2;       /* LPCNET_PLC_CODEC */
constexpr int CONCEAL_OPT_DC_FILTER = 4;   /* LPCNET_PLC_DC_FILTER */

/* PLC_BUF_SIZE (lpcnet_private.h:77); st->pcm holds PLC_BUF_SIZE + FRAME_SIZE shorts */
constexpr int conceal_buf_size(int features_delay) { return features_delay * CONCEAL_FRAME + CONCEAL_HALF; }

/* The control fields of one LPCNetPLCState.  The first CONCEAL_CTRL_INTS, in
 * the order the public state call returns them; feature_buffer_fill is the
 * LPCNetState's inside it.  queued_update follows: only the non-causal mode
 * sets it, and its own state call returns it. */
struct ConcealCtrl {
  int pcm_fill, skip_analysis, blend, loss_count;
  int fec_fill_pos, fec_read_pos, fec_keep_pos, fec_skip;
  int feature_buffer_fill;
  int queued_update;
};
constexpr int CONCEAL_CTRL_INTS = 9;  /* the public layout */
constexpr int CONCEAL_STATE_INTS = 10; /* the whole planner state */
static_assert(sizeof(ConcealCtrl) == CONCEAL_STATE_INTS * sizeof(int), "ConcealCtrl is ten ints, the public nine first");

/* after lpcnet_plc_reset (lpcnet_plc.c:46-59) */
ConcealCtrl conceal_ctrl_reset(int features_delay);

/* One primitive call.  a, b: its parameters, 0 where it has none. */
enum ConcealOp {
  /* the DC filter: remove it from the received frame (:195-204), put it back
   * (:283-287), follow the synthesised frame (:330-335).  a = CDC_*: the
   * non-causal forms keep mem_bak (:363-372), put back dc_buf and lp delayed
   * by half a frame (:444-448), follow one of two ranges (:479-489) */
  CO_DC_REMOVE = 1,
  CO_DC_RESTORE = 2,
  CO_DC_CONCEAL = 3,
  /* burg_cepstral_analysis of the frame into columns 0..35 of the stream's
   * predictor row, flag 1 (:206); a = 1: the row is used as it stands, its
   * feature columns zero (:212-214), a = 0: the analysis fills them (:256) */
  CO_BURG = 4,
  /* preemphasis, compute_frame_features, process_single_frame (:251-254,
   * :324-327): enc.features[0] into columns 36..55 of the row; a = CA_* */
  CO_ANALYSIS = 5,
  /* compute_plc_pred: a = CP_* */
  CO_PREDICT = 6,
  /* plc_copy ring push (:305-306, :313-314); plc_net = plc_copy[a] (:217, :233) */
  CO_PLC_PUSH = 7,
  CO_PLC_RESTORE = 8,
  /* get_fec_or_pred with a queued frame (:149-157): fec[a] into st->features
   * and into the row, flag -1; CO_PREDICT CP_ROW_DISCARD follows */
  CO_FEC_FETCH = 9,
  /* run_frame_network_deferred (lpcnet.c:122-132) of a = CD_*, the buffer
   * holding b frames before the call */
  CO_DEFER_PUSH = 10,
  /* pass a of run_frame_network_flush (lpcnet.c:134-144): run_frame_network
   * of the buffer's frame a, conditioning discarded */
  CO_FLUSH = 11,
  /* lpcnet_synthesize_impl(st->features, ., a, .): b = CI_* */
  CO_IMPL = 12,
  /* lpcnet_synthesize_tail_impl(., a, .): b = CT_* */
  CO_TAIL = 13,
  CO_RESET_SIGNAL = 14, /* :236; clear_state (:404, :175-181) clears the same fields */
  CO_BLEND = 15,        /* :225-229 */
  CO_ATTENUATE = 16,    /* :318-319, a = loss_count */
  /* the st->pcm copies: a = CM_*, b = pcm_fill before the call for CM_APPEND */
  CO_PCM_MOVE = 17,
  /* control only, nothing to launch: fec_rewind(a) (:234), the FEC discard
   * and fec_keep_pos update (:260-262) */
  CO_FEC_REWIND = 18,
  CO_FEC_DISCARD = 19,
  /* the non-causal mode (:339-492) */
  CO_SYN_SAVE = 20,    /* copy = st->lpcnet (:384) */
  CO_SYN_RESTORE = 21, /* st->lpcnet = copy (:414) */
  CO_DC_REDO = 22,     /* :387-400: lp back in, dc_mem = mem_bak, syn_dc over st->pcm[80 .. 160) into dc_mem and delta, lp out again */
  CO_REVERSE = 23,     /* rev[i] = pcm[159 - i] (:403) */
  CO_BLEND_BACK = 24,  /* st->pcm[159 - i] = blend of itself and rev[i] + delta (:407-411) */
  CO_QUEUE_FILL = 25,  /* queued_samples = st->pcm[80 .. 160), pcm[0 .. 80) (:416-418) */
  CO_REORDER = 26,     /* pcm[80 ..) = pcm[0 .. 80), pcm[0 .. 80) = st->pcm[80 ..), st->pcm[0 .. 160) = pcm_save (:440-442) */
  CO_NOPS
};
enum { CP_FULL = 0, CP_BURG_ONLY = 1, CP_ROW_DISCARD = 2, CP_ZERO = 3 };
enum { CD_FEATURES = 0 /* st->features (:221) */, CD_ANALYSED = 1 /* enc.features[0] (:267, :275) */ };
enum {
  CI_BUF = 0,      /* st->pcm[0 .. a) teacher-forced, nothing synthesised (:304-308) */
  CI_SPEC = 1,     /* a samples into tmp, the synthesis state put back afterwards (:223-224, :230) */
  CI_PCM_PRE = 2,  /* the caller's pcm[0 .. a) teacher-forced (:231) */
  CI_PCM_OUT = 3,  /* a samples into the caller's pcm[80 ..) (:320) */
  /* the non-causal mode; st->features unless said otherwise */
  CI_QUEUE = 4,    /* queued_samples[0 .. a) teacher-forced (:344) */
  CI_BUF_OUT = 5,  /* a samples into st->pcm[80 ..) (:385) */
  CI_REV = 6,      /* rev[0 .. a) teacher-forced (:405) */
  CI_ANALYSED = 7, /* enc.features[0]; st->pcm[80 .. 80 + a) teacher-forced (:437) */
  CI_BUF_HI = 8,   /* st->pcm[80 .. 80 + a) teacher-forced (:465) */
  CI_PCM_LO = 9    /* a samples into the caller's pcm[0 ..) (:468) */
};
enum {
  CT_PCM = 0,     /* a samples into the caller's pcm[0 ..) (:315) */
  CT_REV = 1,     /* a samples into rev[0 ..) (:406) */
  CT_PCM_PRE = 2, /* the caller's pcm[0 .. a) teacher-forced, nothing synthesised (:438) */
  CT_PCM_HI = 3   /* a samples into the caller's pcm[80 ..) (:466, :469) */
};
enum {
  CM_TAIL_HALF = 0, /* st->pcm[0 .. 80) = pcm[80 .. 160) (:242, :477) */
  CM_APPEND = 1,    /* st->pcm[pcm_fill ..) = pcm (:245) */
  CM_NEWEST = 2,    /* st->pcm[PLC_BUF_SIZE ..) = pcm (:271) */
  CM_SHIFT = 3,     /* st->pcm moves down by one frame (:280, :309) */
  CM_HEAD_OUT = 4,  /* pcm[0 .. 80) = st->pcm[80 .. 160) (:464) */
  CM_HEAD_IN = 5    /* st->pcm[80 .. 160) = pcm[0 .. 80) (:471) */
};
enum { CA_PCM = 0 /* the caller's pcm */, CA_BUF = 1 /* st->pcm[0 .. 160) (:423-426, :472-475) */ };
enum {
  CDC_CAUSAL = 0,
  CDC_NONCAUSAL = 1, /* CO_DC_REMOVE, CO_DC_RESTORE; CO_DC_CONCEAL over pcm[0 .. 160) (:484) */
  CDC_FIRST_LOSS = 2 /* CO_DC_CONCEAL over pcm[80 .. 160) (:482) */
};

struct ConcealStep {
  int op, a, b;
  bool operator==(const ConcealStep &o) const { return op == o.op && a == o.a && b == o.b; }
  bool operator<(const ConcealStep &o) const { return op != o.op ? op < o.op : a != o.a ? a < o.a : b < o.b; }
};

/* One tick of one stream: lpcnet_plc_update (lost == 0) or lpcnet_plc_conceal.
 * Advances c and appends the tick's steps to `out`.  options: CONCEAL_OPT_*,
 * features_delay 0..CONCEAL_MAX_DELAY, for the non-causal mode 0.  -1 (c and
 * out untouched) for arguments outside that. */
int plan_tick(ConcealCtrl &c, bool lost, int options, int features_delay, std::vector<ConcealStep> &out);

/* lpcnet_plc_fec_add (lpcnet_plc.c:111-128) on the control state.  null_add:
 * fec_skip++.  Otherwise `store` is the row the features go to and, when the
 * queue was compacted first (:121-124), move_from > 0 is the row that became
 * row 0 and move_rows the rows moved.  -1, c untouched: the buffer is full. */
int plan_fec_add(ConcealCtrl &c, bool null_add, int &store, int &move_from, int &move_rows);
void plan_fec_clear(ConcealCtrl &c);

/* The launch sequence of one tick for a batch.  lists[c] is the step list of
 * class c (the streams in one control state that meet the same fate this
 * tick), weight[c] its number of streams.  Every class keeps a cursor into its
 * list; a round takes the classes' next steps and launches each distinct one
 * for all the classes that stand at it -- unless a class that stands elsewhere
 * still has that very step ahead of it: then the step waits for that class,
 * so that lists which differ by a few steps (one flush pass more, one loop
 * pass less) fall back into line and share their synthesis launches.  When
 * every next step waits for another class, the one with the most streams
 * goes.  Streams are independent and a class's own order is kept, so every
 * such merge computes the same.  Control-only steps (CO_FEC_REWIND,
 * CO_FEC_DISCARD) launch nothing and are left out. */
struct ConcealGroup {
  ConcealStep step;
  std::vector<int> classes; /* ascending */
};
std::vector<ConcealGroup> merge_tick(const std::vector<std::vector<ConcealStep>> &lists, const std::vector<int> &weight);

/* what every reachable control state satisfies; false names a planner bug.
 * In the non-causal mode only loss_count, queued_update and the FEC queue's
 * fill side ever leave their reset values. */
bool conceal_ctrl_ok(const ConcealCtrl &c, int features_delay, int options = CONCEAL_OPT_CAUSAL);

}  // namespace lpcnet_mi355x

#endif
