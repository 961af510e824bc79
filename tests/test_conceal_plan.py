"""The concealment machine's planner (lpcnet_amd/csrc/conceal_plan.cpp through
lpcnet_mi355x_conceal_plan, host only) against the restatement of
lpcnet_plc.c's glue (tests/conceal_ref.py, here with stub numerics: only its
trace of primitive calls and its control fields are used), against traces
transcribed by hand from the source text, and on its invariants."""
import itertools

import numpy as np
import pytest

import conceal_ref as CR
import lpcnet_amd as L
from conceal_ref import (ANALYSIS, ATTENUATE, BLEND, BURG, DEFER_PUSH, FEC_DISCARD, FEC_REWIND, FLUSH, IMPL, PCM_MOVE,
                         PLC_PUSH, PLC_RESTORE, PREDICT, RESET_SIGNAL, TAIL)

TICKS = 10


def ref_script(options, delay, lost, events=None):
    """(trace per tick, control fields per tick) of the stub reference."""
    ref = CR.ConcealRef(None, options, delay, stub=True)
    steps, ctrl, k = [], [], 0
    for t, l in enumerate(lost):
        ev = 0 if events is None else int(events[t])
        if ev == -2:
            ref.fec_clear()
        elif ev == -1:
            ref.fec_add(None)
        for _ in range(max(0, ev)):
            ref.fec_add(np.full(20, k, np.float32))
            k += 1
        ref.tick(np.zeros(160, np.int16), bool(l))
        steps.append(ref.take_trace())
        ctrl.append(ref.ctrl())
    return steps, ctrl


def show(steps):
    return [(CR.OP_NAMES[o], a, b) for o, a, b in steps]


@pytest.mark.parametrize("options", [CR.CAUSAL, CR.CODEC], ids=["causal", "codec"])
@pytest.mark.parametrize("delay", [0, 1, 2, 3, 4])
def test_every_pattern_of_ten_ticks(options, delay):
    for pattern in range(1 << TICKS):
        lost = [(pattern >> t) & 1 for t in range(TICKS)]
        want_s, want_c = ref_script(options, delay, lost)
        got_s, got_c = L.conceal_plan(options, delay, lost)
        for t in range(TICKS):
            assert got_s[t] == want_s[t], (pattern, t, show(got_s[t]), show(want_s[t]))
            assert got_c[t] == want_c[t], (pattern, t)


@pytest.mark.parametrize("options", [CR.CAUSAL, CR.CODEC, CR.CAUSAL | CR.DC_FILTER, CR.CODEC | CR.DC_FILTER])
@pytest.mark.parametrize("delay", [0, 1, 2, 3, 4])
def test_the_six_scripts(options, delay):
    lost = CR.lost_matrix()
    fec_seen = False
    for s in range(len(CR.SCRIPTS)):
        ev = CR.fec_events(s)
        want_s, want_c = ref_script(options, delay, lost[s], ev)
        got_s, got_c = L.conceal_plan(options, delay, lost[s], ev)
        assert got_s == want_s and got_c == want_c, s
        fec_seen = fec_seen or any(o == CR.FEC_FETCH for tick in got_s for o, _, _ in tick)
    assert fec_seen, "no script reads a FEC frame"


def test_the_scripts_reach_what_they_are_there_for():
    lost = CR.lost_matrix()
    assert lost.any(0).all() and not lost.all(0).any(), "every tick is a mixed one"
    plans = [L.conceal_plan(CR.CAUSAL, 2, lost[s], CR.fec_events(s)) for s in range(6)]
    flat = [[st for tick in p[0] for st in tick] for p in plans]
    assert not any(o in (IMPL, TAIL, FLUSH) for o, _, _ in flat[0])
    # script 1: skip_analysis counts 3, 2, 1, 0 after the loss
    assert [c["skip_analysis"] for c in plans[1][1][4:9]] == [3, 2, 1, 0, 0]
    # script 2: a loss with skip_analysis > 0 and pcm_fill == 80: the loop runs once with 80
    t = 5
    assert plans[2][1][t - 1]["pcm_fill"] == 80 and plans[2][1][t - 1]["skip_analysis"] > 0
    assert [(a, b) for o, a, b in plans[2][0][t] if o == IMPL] == [(80, CR.CI_BUF), (80, CR.CI_PCM_OUT)]
    # script 3: a loss with pcm_fill == 240: 160 then 80
    t = 9
    assert plans[3][1][t - 1]["pcm_fill"] == 240
    assert [(a, b) for o, a, b in plans[3][0][t] if o == IMPL] == [(160, CR.CI_BUF), (80, CR.CI_BUF), (80, CR.CI_PCM_OUT)]
    # script 4: a loss on the first tick runs the loop over PLC_BUF_SIZE; loss_count reaches 10 and more
    assert [(a, b) for o, a, b in plans[4][0][0] if o == IMPL][:3] == [(160, CR.CI_BUF), (160, CR.CI_BUF), (80, CR.CI_BUF)]
    assert max(c["loss_count"] for c in plans[4][1]) == 12
    assert {a for o, a, _ in flat[4] if o == ATTENUATE} >= {1, 9, 10, 12}
    # script 5: FEC frames read, a tick with the queue dry, and the rewind only in the codec mode
    kinds = [a for o, a, _ in flat[5] if o == PREDICT]
    assert CR.CP_ROW_DISCARD in kinds and CR.CP_ZERO in kinds
    codec = [st for tick in L.conceal_plan(CR.CODEC, 2, lost[5], CR.fec_events(5))[0] for st in tick]
    assert any(o == FEC_REWIND for o, _, _ in codec) and not any(o == FEC_REWIND for o, _, _ in flat[5])


# -- traces transcribed from lpcnet_plc.c, FEATURES_DELAY 2 (PLC_BUF_SIZE 400) ----------------------

G_FIRST = [
    (BURG, 0, 0),                       # :205-206 burg_cepstral_analysis; skip_analysis == 0: :208-248 not taken
    (ANALYSIS, 0, 0),                   # :251-254
    (PREDICT, CR.CP_FULL, 0),           # :255-258, blend == 0
    (FEC_DISCARD, 0, 0),                # :260-262
    (PCM_MOVE, CR.CM_NEWEST, 0),        # :271, the else of :264
    (DEFER_PUSH, CR.CD_ANALYSED, 0),    # :275 run_frame_network_deferred, the buffer empty
    (PCM_MOVE, CR.CM_SHIFT, 0),         # :280
]
L_AFTER_RESET = [
    # :296 run_frame_network_flush: feature_buffer_fill == 0, no frame
    (PLC_PUSH, 0, 0), (PREDICT, CR.CP_ZERO, 0), (IMPL, 160, CR.CI_BUF), (PCM_MOVE, CR.CM_SHIFT, 0),  # :300-311, pcm_fill 400 -> 240
    (PLC_PUSH, 0, 0), (PREDICT, CR.CP_ZERO, 0), (IMPL, 160, CR.CI_BUF), (PCM_MOVE, CR.CM_SHIFT, 0),  # 240 -> 80
    (PLC_PUSH, 0, 0), (PREDICT, CR.CP_ZERO, 0), (IMPL, 80, CR.CI_BUF), (PCM_MOVE, CR.CM_SHIFT, 0),   # 80 -> 0
    (PLC_PUSH, 0, 0),                   # :313-314
    (TAIL, 80, 0),                      # :315
    (PREDICT, CR.CP_ZERO, 0),           # :316 get_fec_or_pred, no FEC: loss_count = 1
    (ATTENUATE, 1, 0),                  # :319
    (IMPL, 80, CR.CI_PCM_OUT),          # :320
    (ANALYSIS, 0, 0),                   # :322-328
]
G_AFTER_L_CAUSAL = [
    (BURG, 1, 0),                       # :206; its row is used with zero features (:212-214)
    (PLC_RESTORE, 2, 0),                # :217 plc_copy[FEATURES_DELAY]
    (PREDICT, CR.CP_BURG_ONLY, 0),      # :218
    (DEFER_PUSH, CR.CD_FEATURES, 0),    # :219-222, twice
    (DEFER_PUSH, CR.CD_FEATURES, 1),
    (IMPL, 80, CR.CI_SPEC),             # :223-224, :230
    (BLEND, 0, 0),                      # :225-229
    (IMPL, 80, CR.CI_PCM_PRE),          # :231
    (PCM_MOVE, CR.CM_TAIL_HALF, 0),     # :242-243
    (ANALYSIS, 0, 0),                   # :251-254; blend == 1: :255-263 not taken
    (DEFER_PUSH, CR.CD_ANALYSED, 2),    # :267
]
G_AFTER_L_CODEC = [
    (BURG, 0, 0),                       # :206
    (PLC_RESTORE, 1, 0),                # :233 plc_copy[FEATURES_DELAY-1]
    (FEC_REWIND, 2, 0),                 # :234
    (RESET_SIGNAL, 0, 0),               # :236
    (PCM_MOVE, CR.CM_TAIL_HALF, 0),     # :242-243
    (ANALYSIS, 0, 0),                   # :251-254; :265 enable_blending == 0: no deferred frame
]


def _ctrl(**kw):
    c = dict.fromkeys(CR.CTRL, 0)
    c.update(kw)
    return c


@pytest.mark.parametrize("who", ["planner", "restatement"])
def test_literal_traces(who):
    def run(options, lost):
        return L.conceal_plan(options, 2, lost) if who == "planner" else ref_script(options, 2, lost)

    for options in (CR.CAUSAL, CR.CODEC):
        s, c = run(options, [0])
        assert s == [G_FIRST] and c == [_ctrl(pcm_fill=400, feature_buffer_fill=1)]
        s, c = run(options, [1])
        assert s == [L_AFTER_RESET] and c == [_ctrl(skip_analysis=3, blend=1, loss_count=1)]
    s, c = run(CR.CAUSAL, [1, 0])
    assert s == [L_AFTER_RESET, G_AFTER_L_CAUSAL] and c[1] == _ctrl(pcm_fill=80, skip_analysis=2, feature_buffer_fill=3)
    s, c = run(CR.CODEC, [1, 0])
    assert s == [L_AFTER_RESET, G_AFTER_L_CODEC] and c[1] == _ctrl(pcm_fill=80, skip_analysis=2)


# -- invariants (tools/conceal_plan_check.cpp asserts the same in C++) ------------------------------

@pytest.mark.parametrize("delay", [0, 1, 2, 3, 4])
def test_invariants(delay):
    buf = CR.plc_buf_size(delay)
    fills = {0} | set(range(80, buf + 1, 160))
    for options, pattern in itertools.product((CR.CAUSAL, CR.CODEC | CR.DC_FILTER), range(0, 1 << TICKS, 3)):
        lost = [(pattern >> t) & 1 for t in range(TICKS)]
        events = [2, 0, -1, 1, 0, 3, 0, -2, 1, 0]
        steps, ctrl = L.conceal_plan(options, delay, lost, events)
        for t in range(TICKS):
            c = ctrl[t]
            assert c["pcm_fill"] in fills
            assert 0 <= c["fec_keep_pos"] <= c["fec_read_pos"] <= c["fec_fill_pos"] <= 100
            assert 0 <= c["feature_buffer_fill"] <= 4
            if not any(lost[:t + 1]):
                assert not any(o in (IMPL, TAIL, FLUSH) for o, _, _ in steps[t])


def test_refusals():
    for options in (CR.NONCAUSAL, 3, 8, CR.NONCAUSAL | CR.DC_FILTER):
        with pytest.raises(L.LPCNetError):
            L.conceal_plan(options, 2, [0, 1])
    for delay in (-1, 5):
        with pytest.raises(L.LPCNetError, match="FEATURES_DELAY"):
            L.conceal_plan(CR.CAUSAL, delay, [0, 1])
    assert L.conceal_plan(CR.CAUSAL, 2, []) == ([], [])
    # 101 adds without a read: the last one is dropped, as the reference drops it
    _, ctrl = L.conceal_plan(CR.CAUSAL, 2, [1], [101])
    assert ctrl[0]["fec_fill_pos"] == 100 and ctrl[0]["fec_read_pos"] == 4  # three loop passes and :316 read one each
