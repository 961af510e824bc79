/*
 * conceal_calls.cpp -- the concealment machine of a batch
 * (lpcnet_batch_conceal_*): lpcnet_plc_update / lpcnet_plc_conceal
 * (lpcnet_plc.c:188-503, causal, codec and non-causal modes) for every stream
 * of a batch in one call per tick, streams that received their packet and
 * streams that lost it side by side.
 *
 * The control state of every stream lives on the host and is advanced by the
 * planner (conceal_plan.cpp) without reading anything back; the data state
 * lives in device memory (ConcealData, lpcnet_engine.h).  A tick plans each
 * stream's ordered step list, merges the lists into one launch sequence --
 * the streams whose next step is the same call with the same parameters form
 * one group (plan_batch_tick) -- and queues every group on b->stream: the glue kernels of
 * conceal_kernel.hip on the group's index list, the predictor, extractor and
 * Burg launches of side_calls.cpp under the group's byte mask, and the
 * synthesis steps on work states: the group's StreamStates gathered into the
 * first n slots of a work array, the step run there (the *_first_device
 * steps of synth_steps.cpp), the states scattered back -- or not, which is the
 * reference's struct copy and restore around a speculative synthesis.  The
 * non-causal mode's copy spans three synthesis calls (:384-414): there the
 * states are saved into an array of their own and put back by explicit steps.
 * Nothing synchronises between the steps or at the end of the device form.
 *
 * The index lists and masks of a tick are written into pinned memory and
 * copied in one transfer before the tick's first launch.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <array>
#include <map>
#include <string>
#include <vector>

#include "batch.h"
#include "conceal_plan.h"

static_assert(CONCEAL_FEC_ROWS == CONCEAL_MAX_FEC && CONCEAL_DEFER == CONCEAL_DEFER_DEPTH && CONCEAL_MAX_DELAY == MAX_FEATURES_DELAY &&
                  CONCEAL_FRAME == FRAME,
              "the planner and the kernels agree on the reference's constants");

#ifndef M_PI
#define M_PI 3.141592653 /* lpcnet_plc.c:35-37 */
#endif

/* ------------------------------------------------------------------------ */
struct ConcealMachine {
  int options = 0;
  ConcealData d{};
  DevPtr<char> base;             /* the carved device buffer */
  StreamState *work = nullptr;   /* [B] the states a synthesis step runs on */
  StreamState *spec = nullptr;   /* [B] lpcnet_plc_update_non_causal's copy (:384, :414); that mode only */
  short *io = nullptr;           /* [B][FRAME] the host form's PCM */
  std::vector<ConcealCtrl> ctrl; /* [B] */
  int ulaw0 = 0;                 /* lin2ulaw(0.f) */
  /* a tick's index lists and masks: built in a pinned slot, one copy into
   * d_lists.  A slot is rewritten once the copy that read it has run. */
  struct Slot {
    PinnedPtr<char> h;
    DevEvent ev;
    bool used = false;
  };
  static constexpr int SLOTS = 4;
  Slot ring[SLOTS];
  int next = 0;
  DevPtr<char> d_lists;
  size_t cap = 0;
  /* what d_lists holds: a tick with the same lists (the steady state: every
   * stream received its packet again) copies nothing */
  std::vector<int> up_idx;
  std::vector<unsigned char> up_mask;
  bool up_valid = false;
};

namespace {

/* a set of streams of one tick: its index list and, where a masked launch
 * asks for it, its byte mask, as offsets into the tick's lists */
struct StreamSet {
  int idx_off = 0, n = 0; /* ints */
  int mask_off = -1;      /* index into the masks, -1: none yet */
};

struct Group {
  ConcealStep step;
  int set; /* index into the tick's sets */
};

/* the plan of one tick for the whole batch */
struct TickPlan {
  std::vector<int> idx;            /* the sets' index lists */
  std::vector<unsigned char> mask; /* [nmasks][B] */
  std::vector<StreamSet> sets;
  std::vector<Group> groups;
};

bool needs_mask(int op) { return op == CO_BURG || op == CO_ANALYSIS || op == CO_PREDICT; }

/* Streams in the same control state that meet the same fate this tick make
 * the same calls: plan once per such class, then merge the classes' lists
 * into one launch sequence (merge_tick, conceal_plan.cpp). */
int plan_batch_tick(const ConcealMachine &M, int B, const unsigned char *lost, const unsigned char *active,
                    std::vector<ConcealCtrl> &ctrl, TickPlan &T)
{
  using Key = std::array<int, CONCEAL_STATE_INTS + 1>;
  struct Class {
    std::vector<int> members;
    std::vector<ConcealStep> steps;
    ConcealCtrl after;
  };
  std::map<Key, int> index;
  std::vector<Class> classes;
  for (int s = 0; s < B; s++) {
    if (active && !active[s]) continue;
    Key k;
    memcpy(k.data(), &ctrl[s], sizeof(ConcealCtrl));
    k[CONCEAL_STATE_INTS] = lost[s] != 0;
    auto it = index.find(k);
    if (it == index.end()) {
      Class c;
      c.after = ctrl[s];
      if (plan_tick(c.after, lost[s] != 0, M.options, M.d.delay, c.steps) || !conceal_ctrl_ok(c.after, M.d.delay, M.options)) {
        set_err("conceal: the planner left its invariants");
        return -1;
      }
      it = index.emplace(k, (int)classes.size()).first;
      classes.push_back(std::move(c));
    }
    classes[it->second].members.push_back(s);
  }
  for (const Class &c : classes)
    for (int s : c.members) ctrl[s] = c.after;
  /* sets of streams, keyed by the classes they unite */
  std::vector<std::vector<ConcealStep>> lists;
  std::vector<int> weight;
  for (const Class &c : classes) {
    lists.push_back(c.steps);
    weight.push_back((int)c.members.size());
  }
  std::map<std::vector<int>, int> set_of;
  for (const ConcealGroup &g : merge_tick(lists, weight)) {
    auto it = set_of.find(g.classes);
    if (it == set_of.end()) {
      StreamSet set;
      set.idx_off = (int)T.idx.size();
      for (int c : g.classes) T.idx.insert(T.idx.end(), classes[c].members.begin(), classes[c].members.end());
      set.n = (int)T.idx.size() - set.idx_off;
      it = set_of.emplace(g.classes, (int)T.sets.size()).first;
      T.sets.push_back(set);
    }
    StreamSet &set = T.sets[it->second];
    if (needs_mask(g.step.op) && set.mask_off < 0 && set.n < B) {
      set.mask_off = (int)(T.mask.size() / B);
      T.mask.resize(T.mask.size() + B, 0);
      for (int i = 0; i < set.n; i++) T.mask[(size_t)set.mask_off * B + T.idx[set.idx_off + i]] = 1;
    }
    T.groups.push_back({g.step, it->second});
  }
  return 0;
}

/* the tick's lists in device memory: one copy from a pinned slot */
int upload_lists(LPCNetBatch *b, ConcealMachine &M, const TickPlan &T, const int *&d_idx, const unsigned char *&d_mask)
{
  const size_t idx_bytes = (T.idx.size() * sizeof(int) + 255) & ~(size_t)255, bytes = idx_bytes + T.mask.size();
  d_idx = (const int *)(char *)M.d_lists;
  d_mask = (const unsigned char *)(char *)M.d_lists + idx_bytes;
  if (M.up_valid && T.idx == M.up_idx && T.mask == M.up_mask) return 0;
  M.up_valid = false;
  if (bytes > M.cap) {
    /* grow: nothing queued may still read the old lists */
    HIPCHK(hipStreamSynchronize(b->stream));
    const size_t cap = std::max(bytes * 2, (size_t)4096);
    M.d_lists.reset();
    M.cap = 0;
    for (ConcealMachine::Slot &s : M.ring) {
      s.h.reset();
      s.used = false;
    }
    if (M.d_lists.alloc(cap)) return -1;
    for (ConcealMachine::Slot &s : M.ring)
      if (s.h.alloc(cap, false)) return -1;
    M.cap = cap;
  }
  ConcealMachine::Slot &s = M.ring[M.next];
  M.next = (M.next + 1) % ConcealMachine::SLOTS;
  if (!s.ev && s.ev.create(false)) return -1;
  if (s.used) HIPCHK(hipEventSynchronize(s.ev)); /* the copy of four ticks ago */
  memcpy(s.h, T.idx.data(), T.idx.size() * sizeof(int));
  if (!T.mask.empty()) memcpy(s.h + idx_bytes, T.mask.data(), T.mask.size());
  if (bytes) HIPCHK(hipMemcpyAsync(M.d_lists, s.h, bytes, hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipEventRecord(s.ev, b->stream));
  s.used = true;
  M.up_idx = T.idx;
  M.up_mask = T.mask;
  M.up_valid = true;
  d_idx = (const int *)(char *)M.d_lists;
  d_mask = (const unsigned char *)(char *)M.d_lists + idx_bytes;
  return 0;
}

int glue(int rc, const char *what)
{
  if (rc) set_err(std::string("conceal: ") + what + " kernel launch failed");
  return rc;
}

/* rows of shorts, one per stream: where a synthesis step takes its teacher
 * forcing from or puts its samples */
struct PcmRows {
  short *p = nullptr;
  int stride = 0, off = 0;
};

/* a synthesis step of a group: its states into the work array, the step
 * there, its PCM where the step says, the states back unless speculative */
int synth_step(LPCNetBatch *b, ConcealMachine &M, const ConcealStep &st, const int *idx, int n, short *d_pcm)
{
  const ConcealData &d = M.d;
  const int N = st.a, row = d.buf + FRAME;
  if (launch_state_copy(M.work, b->d_state, nullptr, idx, n, b->stream)) { set_err("conceal: state gather failed"); return -1; }
  bool commit = true;
  if (st.op == CO_FLUSH) {
    if (st.a < 0 || st.a >= CONCEAL_DEFER) { set_err("conceal: a flush pass outside the deferred buffer"); return -1; }
    if (glue(launch_conceal_gather_rows(idx, n, b->d_feat, d.defer + (size_t)st.a * NF, CONCEAL_DEFER * NF, nullptr, nullptr, 0, 0, b->stream),
             "gather"))
      return -1;
    if (frame_first_device(b, n, b->d_feat, true, M.work)) return -1;
  } else {
    const float *feat = d.features;
    int feat_stride = NF;
    PcmRows pre, out;
    if (st.op == CO_TAIL) {
      feat = nullptr;
      switch (st.b) {
      case CT_PCM: out = {d_pcm, FRAME, 0}; break;
      case CT_REV: out = {d.rev, FRAME, 0}; break;
      case CT_PCM_PRE: pre = {d_pcm, FRAME, 0}; break;
      case CT_PCM_HI: out = {d_pcm, FRAME, FRAME / 2}; break;
      default: set_err("conceal: unknown tail step"); return -1;
      }
    } else { /* CO_IMPL */
      switch (st.b) {
      case CI_BUF: pre = {d.pcm, row, 0}; break;
      case CI_SPEC: out = {d.tmp, FRAME / 2, 0}; commit = false; break;
      case CI_PCM_PRE: pre = {d_pcm, FRAME, 0}; break;
      case CI_PCM_OUT: out = {d_pcm, FRAME, FRAME - N}; break;
      case CI_QUEUE: pre = {d.queued, FRAME, 0}; break;
      case CI_BUF_OUT: out = {d.pcm, row, FRAME / 2}; break;
      case CI_REV: pre = {d.rev, FRAME, 0}; break;
      case CI_ANALYSED: feat = d.rows + BURG_N; feat_stride = PLC_IN; pre = {d.pcm, row, FRAME / 2}; break;
      case CI_BUF_HI: pre = {d.pcm, row, FRAME / 2}; break;
      case CI_PCM_LO: out = {d_pcm, FRAME, 0}; break;
      default: set_err("conceal: unknown synthesis step"); return -1;
      }
    }
    const PcmRows &io = pre.stride ? pre : out;
    if (N < 1 || N > FRAME || !io.p || io.off < 0 || io.off + N > io.stride) { set_err("conceal: a synthesis step outside its rows"); return -1; }
    if (glue(launch_conceal_gather_rows(idx, n, feat ? b->d_feat : nullptr, feat, feat_stride, pre.p ? b->d_pcm : nullptr,
                                        pre.p ? pre.p + pre.off : nullptr, pre.stride, N, b->stream),
             "gather"))
      return -1;
    if (st.op == CO_TAIL ? tail_first_device(b, n, b->d_pcm, N, pre.p ? N : 0, M.work)
                         : synth_first_device(b, n, b->d_feat, b->d_pcm, N, pre.p ? N : 0, M.work))
      return -1;
    if (out.p && glue(launch_conceal_scatter_rows(idx, n, b->d_pcm, out.p + out.off, out.stride, N, b->stream), "scatter")) return -1;
  }
  if (commit && launch_state_copy(b->d_state, M.work, idx, nullptr, n, b->stream)) { set_err("conceal: state scatter failed"); return -1; }
  return 0;
}

int run_group(LPCNetBatch *b, ConcealMachine &M, const ConcealStep &st, const int *idx, int n, const unsigned char *mask, short *d_pcm)
{
  const ConcealData &d = M.d;
  hipStream_t q = b->stream;
  switch (st.op) {
  case CO_DC_REMOVE: return glue(launch_conceal_dc(d, idx, n, d_pcm, st.a == CDC_CAUSAL ? CONCEAL_DC_REMOVE : CONCEAL_DC_REMOVE_BAK, q), "DC");
  case CO_DC_RESTORE:
    if (st.a != CDC_CAUSAL) return glue(launch_conceal_dc_restore_delayed(d, idx, n, d_pcm, q), "DC");
    return glue(launch_conceal_dc(d, idx, n, d_pcm, CONCEAL_DC_RESTORE, q), "DC");
  case CO_DC_CONCEAL:
    return glue(launch_conceal_dc(d, idx, n, d_pcm,
                                  st.a == CDC_CAUSAL ? CONCEAL_DC_CONCEAL : st.a == CDC_FIRST_LOSS ? CONCEAL_DC_CONCEAL_HALF : CONCEAL_DC_CONCEAL_WHOLE,
                                  q),
                "DC");
  case CO_DC_REDO: return glue(launch_conceal_dc(d, idx, n, d_pcm, CONCEAL_DC_REDO, q), "DC");
  case CO_BURG: return burg_launch(b, d_pcm, nullptr, d.rows, PLC_IN, BURG_FILL_FLAG | (st.a ? BURG_FILL_ZERO : 0), 1.f, mask);
  case CO_ANALYSIS:
    if (st.a == CA_BUF) { /* the extractor reads dense [B][FRAME] rows */
      if (glue(launch_conceal_export(d, idx, n, d.frame, 0, 0, FRAME, q), "export")) return -1;
      return feat_launch(b, d.frame, nullptr, d.rows + BURG_N, NF, mask, PLC_IN);
    }
    return feat_launch(b, d_pcm, nullptr, d.rows + BURG_N, NF, mask, PLC_IN);
  case CO_SYN_SAVE:
    if (!M.spec || launch_state_copy(M.spec, b->d_state, idx, idx, n, q)) { set_err("conceal: state save failed"); return -1; }
    return 0;
  case CO_SYN_RESTORE:
    if (!M.spec || launch_state_copy(b->d_state, M.spec, idx, idx, n, q)) { set_err("conceal: state restore failed"); return -1; }
    return 0;
  case CO_REVERSE: return glue(launch_conceal_reverse(d, idx, n, d_pcm, q), "reverse");
  case CO_BLEND_BACK: return glue(launch_conceal_blend_back(d, idx, n, q), "blend");
  case CO_QUEUE_FILL: return glue(launch_conceal_queue_fill(d, idx, n, d_pcm, q), "queue fill");
  case CO_REORDER: return glue(launch_conceal_reorder(d, idx, n, d_pcm, q), "reorder");
  case CO_PREDICT:
    return plc_launch(b, st.a == CP_ZERO ? nullptr : d.rows, st.a == CP_ROW_DISCARD ? nullptr : d.features, mask);
  case CO_PLC_PUSH: return glue(launch_conceal_plc_push(d, idx, n, q), "plc_copy");
  case CO_PLC_RESTORE: return glue(launch_conceal_plc_restore(d, idx, n, st.a, q), "plc_copy");
  case CO_FEC_FETCH: return glue(launch_conceal_fec_fetch(d, idx, n, st.a, q), "FEC fetch");
  case CO_DEFER_PUSH: return glue(launch_conceal_defer_push(d, idx, n, st.a == CD_ANALYSED, st.b, q), "deferred push");
  case CO_FLUSH:
  case CO_IMPL:
  case CO_TAIL: return synth_step(b, M, st, idx, n, d_pcm);
  case CO_RESET_SIGNAL: return glue(launch_conceal_reset_signal(b->d_state, idx, n, M.ulaw0, q), "reset_signal");
  case CO_BLEND: return glue(launch_conceal_blend(d, idx, n, d_pcm, q), "blend");
  case CO_ATTENUATE: return glue(launch_conceal_attenuate(d, idx, n, st.a, q), "attenuation");
  case CO_PCM_MOVE:
    switch (st.a) {
    case CM_TAIL_HALF: return glue(launch_conceal_move(d, idx, n, d_pcm, 0, 0, FRAME / 2, FRAME / 2, q), "move");
    case CM_APPEND: return glue(launch_conceal_move(d, idx, n, d_pcm, st.b, 0, 0, FRAME, q), "move");
    case CM_NEWEST: return glue(launch_conceal_move(d, idx, n, d_pcm, d.buf, 0, 0, FRAME, q), "move");
    case CM_SHIFT: return glue(launch_conceal_move(d, idx, n, nullptr, 0, 1, FRAME, d.buf, q), "move");
    case CM_HEAD_OUT: return glue(launch_conceal_export(d, idx, n, d_pcm, 0, FRAME / 2, FRAME / 2, q), "move");
    case CM_HEAD_IN: return glue(launch_conceal_move(d, idx, n, d_pcm, FRAME / 2, 0, 0, FRAME / 2, q), "move");
    }
  }
  set_err("conceal: unknown step");
  return -1;
}

int machine_ready(LPCNetBatch *b)
{
  if (!b) { set_err("null batch"); return -1; }
  if (!b->conceal) { set_err("conceal: no machine open on this batch (lpcnet_batch_conceal_open)"); return -1; }
  return 0;
}

/* one tick on device PCM, queued */
int tick(LPCNetBatch *b, short *d_pcm, const unsigned char *lost, const unsigned char *active)
{
  ConcealMachine &M = *b->conceal;
  if (b->mc.delay != M.d.delay) {
    set_err("conceal: FEATURES_DELAY changed since lpcnet_batch_conceal_open; close and reopen the machine");
    return -1;
  }
  std::vector<ConcealCtrl> ctrl = M.ctrl;
  TickPlan T;
  if (plan_batch_tick(M, b->B, lost, active, ctrl, T)) return -1;
  if (T.groups.empty()) return 0;
  const int *d_idx;
  const unsigned char *d_mask;
  if (upload_lists(b, M, T, d_idx, d_mask)) return -1;
  /* a call that fails from here on has queued a part of the tick: the
   * streams' states are then undefined until a reset, as after any failed
   * launch; the control state stays the tick's start */
  for (const Group &g : T.groups) {
    const StreamSet &set = T.sets[g.set];
    if (run_group(b, M, g.step, d_idx + set.idx_off, set.n, set.mask_off < 0 ? nullptr : d_mask + (size_t)set.mask_off * b->B, d_pcm))
      return -1;
  }
  M.ctrl.swap(ctrl);
  return 0;
}

}  // namespace

/* ------------------------------------------------------------------------ */
namespace lpcnet_mi355x {

void conceal_free(LPCNetBatch *b)
{
  ConcealMachine *M = b->conceal;
  if (!M) return;
  (void)hipStreamSynchronize(b->stream);
  delete M;
  b->conceal = nullptr;
}

/* lpcnet_plc_reset (lpcnet_plc.c:46-59) beyond what the batch's reset does
 * already (lpcnet_reset, plc_net, lpcnet_encoder_init): the RNN_CLEAR from
 * fec to the end of the struct, pcm_fill = PLC_BUF_SIZE */
int conceal_reset_streams(LPCNetBatch *b, int stream)
{
  ConcealMachine *M = b->conceal;
  if (!M) return 0;
  const ConcealData &d = M->d;
  const size_t first = stream < 0 ? 0 : (size_t)stream, n = stream < 0 ? (size_t)b->B : 1;
  std::vector<StateRows> rows = {{d.features, NF * 4},
                                 {d.pcm, (size_t)(d.buf + FRAME) * 2},
                                 {d.dc, 16},
                                 {d.copy, (size_t)(d.delay + 1) * d.nt * 4},
                                 {d.fec, (size_t)CONCEAL_FEC_ROWS * NF * 4},
                                 {d.defer, (size_t)CONCEAL_DEFER * NF * 4},
                                 {d.delta, 4}};
  if (d.queued) { /* the non-causal mode: queued_samples, dc_buf */
    rows.push_back({d.queued, FRAME * 2});
    rows.push_back({d.dc_buf, FRAME / 2 * 2});
  }
  if (rows_zero(rows, stream, b->B, b->stream)) return -1;
  for (size_t s = first; s < first + n; s++) M->ctrl[s] = conceal_ctrl_reset(d.delay);
  return 0;
}

}  // namespace lpcnet_mi355x

extern "C" {

LPCNET_EXPORT int lpcnet_batch_conceal_open(LPCNetBatch *b, int options)
{
  if (plc_ready(b)) return -1;
  if ((options & ~7) || (options & 3) == 3) { set_err("conceal: options must be LPCNET_CONCEAL_CAUSAL, _NONCAUSAL or _CODEC, with or without _DC_FILTER"); return -1; }
  const bool noncausal = (options & 3) == CONCEAL_OPT_NONCAUSAL;
  if (noncausal && b->mc.delay != 0) { /* the reference exits (:357-361) */
    set_err("conceal: the non-causal mode (LPCNET_PLC_NONCAUSAL) needs a model with FEATURES_DELAY 0 "
            "(lpcnet_batch_set_model_constants or the blob's record); this batch has " + std::to_string(b->mc.delay));
    return -1;
  }
  if (b->conceal) { set_err("conceal: a machine is already open on this batch"); return -1; }
  if (b->set_device() || burg_ensure(b)) return -1;
  const size_t B = (size_t)b->B;
  auto M = std::make_unique<ConcealMachine>();
  M->options = options;
  M->ctrl.resize(B);
  StreamState r;
  host_reset_state(r);
  M->ulaw0 = r.last_exc;
  ConcealData &d = M->d;
  d.nstreams = b->B;
  d.delay = b->mc.delay;
  d.buf = conceal_buf_size(d.delay);
  d.nt = b->pa.n1 + b->pa.n2;
  d.plc_state = b->plc.state;
  float *w = nullptr;
  Carver c;
  c.add(d.features, B * NF);
  c.add(d.pcm, B * (d.buf + FRAME));
  c.add(d.dc, B * 2);
  c.add(d.copy, B * (d.delay + 1) * d.nt);
  c.add(d.fec, B * CONCEAL_FEC_ROWS * NF);
  c.add(d.defer, B * CONCEAL_DEFER * NF);
  c.add(d.rows, B * PLC_IN);
  c.add(d.lp, B * FRAME);
  c.add(d.delta, B);
  c.add(d.tmp, B * (FRAME / 2));
  c.add(w, FRAME / 2);
  c.add(M->work, B);
  c.add(M->io, B * FRAME);
  if (noncausal) {
    c.add(M->spec, B);
    c.add(d.mem_bak, B);
    c.add(d.queued, B * FRAME);
    c.add(d.dc_buf, B * (FRAME / 2));
    c.add(d.rev, B * FRAME);
    c.add(d.frame, B * FRAME);
  }
  /* the blend window as the reference computes it per sample (:227), the host's cos */
  float win[FRAME / 2];
  for (int i = 0; i < FRAME / 2; i++) win[i] = (float)(.5 - .5 * cos(M_PI * i / (FRAME / 2)));
  M->base = c.alloc();
  if (!M->base || hipMemsetAsync(M->base, 0, c.size(), b->stream) != hipSuccess ||
      hipMemcpyAsync(w, win, sizeof(win), hipMemcpyHostToDevice, b->stream) != hipSuccess ||
      hipStreamSynchronize(b->stream) != hipSuccess) { /* win leaves scope */
    set_err("conceal: device allocation failed");
    return -1;
  }
  d.blend_w = w;
  b->conceal = M.release();
  lpcnet_batch_reset(b); /* lpcnet_plc_init + lpcnet_plc_reset for every stream */
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_conceal_close(LPCNetBatch *b)
{
  if (machine_ready(b) || b->set_device()) return -1;
  conceal_free(b);
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_conceal_reset(LPCNetBatch *b, int stream)
{
  if (machine_ready(b)) return -1;
  if (stream < -1 || stream >= b->B) { set_err("no such stream"); return -1; }
  if (stream < 0) {
    lpcnet_batch_reset(b);
    return 0;
  }
  return lpcnet_batch_reset_stream(b, stream);
}

LPCNET_EXPORT int lpcnet_batch_conceal_frame_device(LPCNetBatch *b, short *d_pcm, const unsigned char *lost, const unsigned char *active)
{
  if (machine_ready(b)) return -1;
  if (!d_pcm || !lost) { set_err("bad arguments"); return -1; }
  if (plc_ready(b) || b->set_device()) return -1;
  return tick(b, d_pcm, lost, active);
}

LPCNET_EXPORT int lpcnet_batch_conceal_frame(LPCNetBatch *b, short *pcm, const unsigned char *lost, const unsigned char *active)
{
  if (machine_ready(b)) return -1;
  if (!pcm || !lost) { set_err("bad arguments"); return -1; }
  if (plc_ready(b) || b->set_device()) return -1;
  ConcealMachine &M = *b->conceal;
  const size_t B = (size_t)b->B, row = FRAME * sizeof(short);
  HIPCHK(hipMemcpyAsync(M.io, pcm, B * row, hipMemcpyHostToDevice, b->stream));
  if (tick(b, M.io, lost, active)) return -1;
  std::vector<short> out(B * FRAME);
  HIPCHK(hipMemcpyAsync(out.data(), M.io, B * row, hipMemcpyDeviceToHost, b->stream));
  if (lpcnet_batch_sync(b)) return -1;
  for (size_t s = 0; s < B; s++)
    if (!active || active[s]) memcpy(pcm + s * FRAME, &out[s * FRAME], row);
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_conceal_fec_add(LPCNetBatch *b, int stream, const float *features)
{
  if (machine_ready(b)) return -1;
  if (stream < 0 || stream >= b->B) { set_err("no such stream"); return -1; }
  if (b->set_device()) return -1;
  ConcealMachine &M = *b->conceal;
  ConcealCtrl c = M.ctrl[stream];
  int store, from, rows;
  if (plan_fec_add(c, features == nullptr, store, from, rows)) { set_err("FEC buffer full"); return -1; }
  if (rows > 0 && launch_conceal_fec_compact(M.d, stream, from, rows, b->stream)) { set_err("conceal: FEC compaction kernel launch failed"); return -1; }
  if (store >= 0 && launch_conceal_fec_store(M.d, stream, store, features, b->stream)) { set_err("conceal: FEC store kernel launch failed"); return -1; }
  M.ctrl[stream] = c;
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_conceal_fec_clear(LPCNetBatch *b, int stream)
{
  if (machine_ready(b)) return -1;
  if (stream < 0 || stream >= b->B) { set_err("no such stream"); return -1; }
  plan_fec_clear(b->conceal->ctrl[stream]);
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_conceal_get_state(LPCNetBatch *b, int stream, int *ctrl, float *features, short *pcm_buf, double *dc)
{
  if (machine_ready(b)) return -1;
  if (stream < 0 || stream >= b->B) { set_err("no such stream"); return -1; }
  if (!ctrl || !features || !pcm_buf || !dc) { set_err("bad arguments"); return -1; }
  if (b->set_device()) return -1;
  const ConcealMachine &M = *b->conceal;
  const ConcealData &d = M.d;
  HIPCHK(hipStreamSynchronize(b->stream));
  memcpy(ctrl, &M.ctrl[stream], CONCEAL_CTRL_INTS * sizeof(int));
  const size_t s = (size_t)stream, np = (size_t)d.buf + FRAME;
  HIPCHK(hipMemcpy(features, d.features + s * NF, NF * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(pcm_buf, d.pcm + s * np, np * 2, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(dc, d.dc + s * 2, 16, hipMemcpyDeviceToHost));
  return 0;
}

LPCNET_EXPORT int lpcnet_batch_conceal_get_state_noncausal(LPCNetBatch *b, int stream, int *queued_update, short *queued_samples, short *dc_buf)
{
  if (machine_ready(b)) return -1;
  if (stream < 0 || stream >= b->B) { set_err("no such stream"); return -1; }
  const ConcealMachine &M = *b->conceal;
  if ((M.options & 3) != CONCEAL_OPT_NONCAUSAL) { set_err("conceal: the open machine is not in the non-causal mode"); return -1; }
  if (b->set_device()) return -1;
  HIPCHK(hipStreamSynchronize(b->stream));
  const size_t s = (size_t)stream;
  if (queued_update) *queued_update = M.ctrl[stream].queued_update;
  if (queued_samples) HIPCHK(hipMemcpy(queued_samples, M.d.queued + s * FRAME, FRAME * 2, hipMemcpyDeviceToHost));
  if (dc_buf) HIPCHK(hipMemcpy(dc_buf, M.d.dc_buf + s * (FRAME / 2), FRAME / 2 * 2, hipMemcpyDeviceToHost));
  return 0;
}

/* Host only: the planner over a script of one stream from reset (tests, tools). */
LPCNET_EXPORT int lpcnet_mi355x_conceal_plan(int options, int features_delay, const unsigned char *lost, const int *fec_adds, int nticks,
                                             int *steps, int max_steps, int *tick_end, int *ctrl)
{
  if (nticks < 0 || (nticks > 0 && !lost) || max_steps < 0 || (max_steps > 0 && !steps)) { set_err("bad arguments"); return -1; }
  if (features_delay < 0 || features_delay > CONCEAL_MAX_DELAY) { set_err("conceal plan: FEATURES_DELAY outside 0..4"); return -1; }
  if ((options & ~7) == 0 && (options & 3) == CONCEAL_OPT_NONCAUSAL && features_delay != 0) {
    set_err("conceal plan: the non-causal mode needs FEATURES_DELAY 0");
    return -1;
  }
  ConcealCtrl c = conceal_ctrl_reset(features_delay);
  std::vector<ConcealStep> all;
  for (int t = 0; t < nticks; t++) {
    const int ev = fec_adds ? fec_adds[t] : 0;
    int store, from, rows;
    if (ev == -2) plan_fec_clear(c);
    else if (ev == -1) (void)plan_fec_add(c, true, store, from, rows);
    for (int k = 0; k < ev; k++) (void)plan_fec_add(c, false, store, from, rows); /* a full buffer drops the add (:118-119) */
    if (plan_tick(c, lost[t] != 0, options, features_delay, all)) { set_err("conceal plan: options outside the causal, non-causal and codec modes"); return -1; }
    if (tick_end) tick_end[t] = (int)all.size();
    if (ctrl) memcpy(ctrl + (size_t)t * CONCEAL_CTRL_INTS, &c, CONCEAL_CTRL_INTS * sizeof(int));
  }
  if (!steps) return (int)all.size(); /* the count alone */
  if ((int)all.size() > max_steps) { set_err("conceal plan: more steps than max_steps"); return -1; }
  for (size_t k = 0; k < all.size(); k++) {
    steps[3 * k] = all[k].op;
    steps[3 * k + 1] = all[k].a;
    steps[3 * k + 2] = all[k].b;
  }
  return (int)all.size();
}

}  // extern "C"
