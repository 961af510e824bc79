"""The concealment planner in the non-causal mode (lpcnet_amd/csrc/conceal_plan.cpp
through lpcnet_mi355x_conceal_plan, host only) against the restatement of
lpcnet_plc.c:342-492 (tests/conceal_nc_ref.py with stub numerics: only its
trace of primitive calls and its control fields are used), against traces
transcribed by hand from the source text, and on what the fixture's scripts
are there to reach."""
import numpy as np
import pytest

import conceal_nc_ref as NR
import conceal_ref as CR
import lpcnet_amd as L
from conceal_nc_ref import (BLEND_BACK, CA_BUF, CA_PCM, CDC_FIRST_LOSS, CDC_NONCAUSAL, CI_ANALYSED, CI_BUF_HI, CI_BUF_OUT,
                            CI_PCM_LO, CI_QUEUE, CI_REV, CM_HEAD_IN, CM_HEAD_OUT, CT_PCM_HI, CT_PCM_PRE, CT_REV, DC_REDO,
                            QUEUE_FILL, REORDER, REVERSE, SYN_RESTORE, SYN_SAVE)
from conceal_ref import (ANALYSIS, ATTENUATE, BURG, DC_CONCEAL, DC_REMOVE, DC_RESTORE, FEC_FETCH, IMPL, PCM_MOVE, PREDICT,
                         RESET_SIGNAL, TAIL)

TICKS = 10
NC, NC_DC = CR.NONCAUSAL, CR.NONCAUSAL | CR.DC_FILTER


def ref_script(options, lost, events=None):
    """(trace per tick, control fields per tick, queued_update per tick) of the stub restatement."""
    ref = NR.ConcealNcRef(None, options, stub=True)
    steps, ctrl, queued = [], [], []
    for t, l in enumerate(lost):
        ev = 0 if events is None else int(events[t])
        if ev == -2:
            ref.fec_clear()
        elif ev == -1:
            ref.fec_add(None)
        for _ in range(max(0, ev)):
            ref.fec_add(np.zeros(20, np.float32))
        ref.tick(np.zeros(160, np.int16), bool(l))
        steps.append(ref.take_trace())
        ctrl.append(ref.ctrl())
        queued.append(ref.queued_update)
    return steps, ctrl, queued


def names(steps):
    return [((CR.OP_NAMES[o] if o < len(CR.OP_NAMES) else NR.OP_NAMES[o]), a, b) for o, a, b in steps]


@pytest.mark.parametrize("options", [NC, NC_DC], ids=["plain", "dc"])
def test_every_pattern_of_ten_ticks(options):
    for pattern in range(1 << TICKS):
        lost = [(pattern >> t) & 1 for t in range(TICKS)]
        want_s, want_c, _ = ref_script(options, lost)
        got_s, got_c = L.conceal_plan(options, 0, lost)
        for t in range(TICKS):
            assert got_s[t] == want_s[t], (pattern, t, names(got_s[t]), names(want_s[t]))
            assert got_c[t] == want_c[t], (pattern, t)


@pytest.mark.parametrize("options", [NC, NC_DC], ids=["plain", "dc"])
def test_the_six_scripts(options):
    lost = CR.lost_matrix()
    for s in range(len(CR.SCRIPTS)):
        ev = CR.fec_events(s)
        want_s, want_c, _ = ref_script(options, lost[s], ev)
        got_s, got_c = L.conceal_plan(options, 0, lost[s], ev)
        assert got_s == want_s and got_c == want_c, s


def test_the_scripts_reach_what_they_are_there_for():
    lost = CR.lost_matrix()
    plans = [L.conceal_plan(NC_DC, 0, lost[s], CR.fec_events(s)) for s in range(6)]
    queued = [ref_script(NC_DC, lost[s], CR.fec_events(s))[2] for s in range(6)]
    flat = [[st for tick in p[0] for st in tick] for p in plans]

    def consumes_queue(s, t):
        return plans[s][0][t][0] == (IMPL, 160, CI_QUEUE)

    # script 4: a loss from reset takes :467-476 with nothing queued and nothing ever received; loss_count >= 10
    assert lost[4, 0] and plans[4][0][0][0] == (PREDICT, CR.CP_ZERO, 0) and (PCM_MOVE, CM_HEAD_OUT, 0) in plans[4][0][0]
    assert max(c["loss_count"] for c in plans[4][1]) == 12
    assert {a for o, a, _ in flat[4] if o == ATTENUATE} >= {0, 1, 9, 10, 11}
    # scripts 1 and 2: a received tick straight after a loss queues an update, the next received tick consumes it
    for s, t in ((1, 5), (2, 4)):
        assert lost[s, t - 1] and not lost[s, t] and queued[s][t] == 1 and (QUEUE_FILL, 0, 0) in plans[s][0][t]
    assert not lost[1, 6] and consumes_queue(1, 6) and queued[1][6] == 0
    # script 2 and script 3's LG run: the queue consumed by a conceal
    assert lost[2, 5] and consumes_queue(2, 5)
    t = 16  # "LG" * 6 starts at tick 16
    assert CR.SCRIPTS[3][t:t + 4] == "LGLG" and queued[3][t + 1] == 1 and lost[3, t + 2] and consumes_queue(3, t + 2)
    # a second lost tick in a row: :468-475, the analysis of st->pcm
    assert lost[2, 2] and lost[2, 3] and (IMPL, 80, CI_PCM_LO) in plans[2][0][3] and (ANALYSIS, CA_BUF, 0) in plans[2][0][3]
    # script 5 ends on a lost tick; its FEC events move the queue's positions and nothing else
    assert lost[5, -1] and plans[5][1][-1]["loss_count"] > 0
    assert plans[5][1][9]["fec_fill_pos"] > 0 and plans[5][1][9]["fec_read_pos"] == 0 and plans[5][1][10]["fec_fill_pos"] == 0
    assert not any(o == FEC_FETCH for o, _, _ in flat[5])
    assert plans[5][0] == L.conceal_plan(NC_DC, 0, lost[5])[0], "FEC events changed a non-causal tick"
    assert any(c["fec_skip"] for c in plans[5][1])
    # the other control fields never leave their reset values
    for p in plans:
        for c in p[1]:
            assert (c["pcm_fill"], c["skip_analysis"], c["blend"], c["feature_buffer_fill"], c["fec_read_pos"], c["fec_keep_pos"]) == \
                (80, 0, 0, 0, 0, 0)


# -- traces transcribed from lpcnet_plc.c:342-492, with the DC filter (the steps marked dc drop out without it) --

G_FIRST = [
    # :362 process_queued_update: nothing queued
    (DC_REMOVE, CDC_NONCAUSAL, 0),      # dc :363-372, mem_bak kept
    (BURG, 0, 0),                       # :373-375; loss_count == 0: :377-428 not taken
    (ANALYSIS, CA_PCM, 0),              # :429-432
    (PREDICT, CR.CP_FULL, 0),           # :434-436
    (IMPL, 80, CI_ANALYSED),            # :437 enc.features[0], st->pcm[80..160) teacher-forced
    (TAIL, 80, CT_PCM_PRE),             # :438 pcm[0..80) teacher-forced
    (REORDER, 0, 0),                    # :440-442
    (DC_RESTORE, CDC_NONCAUSAL, 0),     # dc :444-448
]
L_FIRST = [
    # :456 nothing queued
    (PREDICT, CR.CP_ZERO, 0),           # :459
    (ATTENUATE, 0, 0),                  # :460-461 with loss_count before its increment (:490)
    (PCM_MOVE, CM_HEAD_OUT, 0),         # :464, the loss_count == 0 branch: no analysis step
    (IMPL, 80, CI_BUF_HI),              # :465
    (TAIL, 80, CT_PCM_HI),              # :466
    (PCM_MOVE, CR.CM_TAIL_HALF, 0),     # :477
    (DC_CONCEAL, CDC_FIRST_LOSS, 0),    # dc :479-489, syn_dc over pcm[80..160) (:482)
]
G_AFTER_L = [
    (DC_REMOVE, CDC_NONCAUSAL, 0),      # dc :363-372
    (BURG, 1, 0),                       # :373-375; the row is used with zero features (:380-382)
    (PREDICT, CR.CP_BURG_ONLY, 0),      # :383
    (SYN_SAVE, 0, 0),                   # :384
    (IMPL, 80, CI_BUF_OUT),             # :385 into st->pcm[80..160)
    (DC_REDO, 0, 0),                    # dc :387-400
    (REVERSE, 0, 0),                    # :403
    (RESET_SIGNAL, 0, 0),               # :404 clear_state
    (IMPL, 160, CI_REV),                # :405
    (TAIL, 80, CT_REV),                 # :406
    (BLEND_BACK, 0, 0),                 # :407-411
    (SYN_RESTORE, 0, 0),                # :414
    (QUEUE_FILL, 0, 0),                 # :416-418
    (ANALYSIS, CA_BUF, 0),              # :423-426
    (ANALYSIS, CA_PCM, 0),              # :429-432; loss_count > 0: no CP_FULL prediction, :433-439 not taken
    (REORDER, 0, 0),                    # :440-442
    (DC_RESTORE, CDC_NONCAUSAL, 0),     # dc :444-448
]
G_WITH_QUEUE = [(IMPL, 160, CI_QUEUE)] + G_FIRST  # :362, :342-347
L_SECOND = [
    (PREDICT, CR.CP_ZERO, 0),           # :459
    (ATTENUATE, 1, 0),                  # :460-461
    (IMPL, 80, CI_PCM_LO),              # :468
    (TAIL, 80, CT_PCM_HI),              # :469
    (PCM_MOVE, CM_HEAD_IN, 0),          # :471
    (ANALYSIS, CA_BUF, 0),              # :472-475
    (PCM_MOVE, CR.CM_TAIL_HALF, 0),     # :477
    (DC_CONCEAL, CDC_NONCAUSAL, 0),     # dc :479-489, syn_dc over the whole frame (:484)
]
DC_STEPS = (DC_REMOVE, DC_RESTORE, DC_CONCEAL, DC_REDO)


def _ctrl(**kw):
    c = dict.fromkeys(CR.CTRL, 0)
    c["pcm_fill"] = 80
    c.update(kw)
    return c


@pytest.mark.parametrize("who", ["planner", "restatement"])
@pytest.mark.parametrize("options", [NC, NC_DC], ids=["plain", "dc"])
def test_literal_traces(who, options):
    def run(lost):
        return L.conceal_plan(options, 0, lost) if who == "planner" else ref_script(options, lost)[:2]

    def tr(steps):
        return steps if options & CR.DC_FILTER else [st for st in steps if st[0] not in DC_STEPS]

    s, c = run([0])
    assert s == [tr(G_FIRST)] and c == [_ctrl()]
    s, c = run([1])
    assert s == [tr(L_FIRST)] and c == [_ctrl(loss_count=1)]
    assert not any(o == ANALYSIS for o, _, _ in s[0])
    s, c = run([1, 0, 0])
    assert s == [tr(L_FIRST), tr(G_AFTER_L), tr(G_WITH_QUEUE)] and c[1] == _ctrl() and c[2] == _ctrl()
    assert not any(st == (PREDICT, CR.CP_FULL, 0) for st in s[1])
    s, c = run([1, 1])
    assert s == [tr(L_FIRST), tr(L_SECOND)] and c[1] == _ctrl(loss_count=2)


def test_refusals():
    for options in (NC, NC_DC):
        for delay in (1, 2, 3, 4):
            with pytest.raises(L.LPCNetError, match="non-causal"):
                L.conceal_plan(options, delay, [0, 1])
    with pytest.raises(L.LPCNetError, match="options"):
        L.conceal_plan(3, 0, [0])
    with pytest.raises(ValueError):
        NR.ConcealNcRef(None, CR.CAUSAL, stub=True)
    assert L.conceal_plan(NC, 0, []) == ([], [])


@pytest.mark.parametrize("options", [NC, NC_DC], ids=["plain", "dc"])
def test_step_counts_without_a_loss(options):
    """An all-received tick: exactly one impl of 80 and one tail of 80 -- one
    frame of teacher-forced synthesis -- and nothing speculative."""
    steps, _ = L.conceal_plan(options, 0, CR.lost_matrix()[0])
    for tick in steps:
        assert [(a, b) for o, a, b in tick if o == IMPL] == [(80, CI_ANALYSED)]
        assert [(a, b) for o, a, b in tick if o == TAIL] == [(80, CT_PCM_PRE)]
        assert not any(o in (SYN_SAVE, SYN_RESTORE, REVERSE, BLEND_BACK, QUEUE_FILL, RESET_SIGNAL, DC_REDO) for o, _, _ in tick)
