"""The concealment machine on its edge cases (tests/conceal_edge.py) against
the fixture tests/golden/conceal_edge.npz, bit for bit in the PCM of every
tick and in the final state of every stream: every FEATURES_DELAY the other
fixtures leave out (set D), PCM that wraps the DC filter's short stores and
drives dc_mem to both ends of int16 (set E), FEC rows that are not ordinary
features (set F); the deeper rings and longer st->pcm rows inside a larger
batch; groups of more than one workgroup of the lane-per-stream kernels, with
active masks that leave one stream or drop every fourth; and a reset in the
middle of a burst at FEATURES_DELAY 4."""
import functools

import numpy as np
import pytest

import conceal_edge as CE
import conceal_ref as CR
import lpcnet_amd as L
import test_gpu_conceal as TG
import test_gpu_conceal_nc as TN

pytestmark = pytest.mark.gpu

NS = len(CR.SCRIPTS)


def open_batch(B, run):
    _, options, delay = CE.RUN[run]
    b = L.LPCNetBatch(B, 0, CE.model_blob())
    if delay != 2:
        b.set_model_constants(1.0, delay, False)
    b.conceal_open(options)
    return b


@functools.lru_cache(maxsize=None)
def table(run):
    return CE.run_inputs(run)


class Driver:
    """tests/test_gpu_conceal.py's driver (the non-causal one in that mode) on
    a run of the edge fixture: stream s plays case cases[s] of the run."""

    def __init__(self, b, run, cases, device):
        fx = table(run)
        self.run, self.nc = run, CE.RUN[run][1] & 3 == CR.NONCAUSAL
        if self.nc:
            self.d = TN.Driver(b, run, cases, device, fx=fx)
        else:
            self.d = TG.Driver(b, cases, device, fx=fx, rows=lambda c, k: fx["rows"][c, k])
        self.tick, self.restart, self.close = self.d.tick, self.d.restart, self.d.close

    def want(self, s, t):
        return self.d.want(s, t) if self.nc else self.d.want(self.run, s, t)


def play(b, run, cases, device, ticks=CR.NTICKS):
    d = Driver(b, run, cases, device)
    for t in range(ticks):
        _, out = d.tick()
        for s, c in enumerate(cases):
            assert np.array_equal(out[s], d.want(s, t)), (run, "tick", t, "stream", s, "case", c)
    return d


# -- 1. sets D, E and F ----------------------------------------------------------------------------------

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("run", [r[0] for r in CE.RUNS])
def test_runs_against_fixture(require_gpu, run, device):
    S = CE.nstreams(run)
    b = open_batch(S, run)
    d = play(b, run, range(S), device)
    for s in range(S):
        CE.check_final_state(b, run, s, s)
    d.close()


# -- 2. the longer st->pcm rows and deeper rings do not depend on the stream index -------------------------

@pytest.mark.parametrize("run", ["d_causal_dc_1", "d_causal_3", "d_causal_dc_4"])
def test_delays_inside_a_larger_batch(require_gpu, run):
    """19 streams on the six scripts cyclically, the shape of
    tests/test_gpu_conceal.py's grouping test: rows of 400, 720 and 880 shorts
    and rings of 2, 4 and 5 predictor states per stream."""
    B = 19
    cases = [s % NS for s in range(B)]
    b = open_batch(B, run)
    d = play(b, run, cases, True)
    for s in range(B):
        CE.check_final_state(b, run, s, cases[s])
    d.close()


# -- 3. group shapes -------------------------------------------------------------------------------------

GROUP_TICKS = 12


def masked_tick(d, b, run, active):
    """One tick under an active mask: the active streams give their fixture
    rows, the inactive ones keep row and state."""
    B = b.B
    idle = np.flatnonzero(~active)
    before = [TG.snapshots(b, s) for s in idle]
    at = d.pos.copy()
    given, out = d.tick(active)
    for s in range(B):
        if active[s]:
            assert np.array_equal(out[s], d.want(run, s, at[s])), (s, at[s])
        else:
            assert np.array_equal(out[s], given[s]), ("the row of an inactive stream changed", s)
    assert [TG.snapshots(b, s) for s in idle] == before, "the state of an inactive stream changed"


@pytest.mark.parametrize("B", [65, 130])
def test_group_shapes(require_gpu, B):
    """tests/golden/conceal.npz's causal_dc run, the six scripts cyclically
    over their first 12 ticks: the DC filter's and the attenuation's groups
    pass 64 streams, one lane of a second block at 65.  At 130, stream 129
    takes its tick 3 alone (a lost tick of script 3: a group of one at the
    highest index) and a later tick leaves out every fourth stream; the
    streams left out catch up at the end."""
    run = "causal_dc"
    b = TG.open_batch(B, run)
    d = TG.Driver(b, [s % NS for s in range(B)], True)
    g = 0
    while (d.pos < GROUP_TICKS).any():
        todo = d.pos < GROUP_TICKS
        if B == 130 and g == 3:
            only = np.zeros(B, bool)
            only[B - 1] = True
            assert d.fx["lost"][(B - 1) % NS, d.pos[B - 1]]
            masked_tick(d, b, run, only)
        elif B == 130 and g == 6:
            masked_tick(d, b, run, todo & (np.arange(B) % 4 != 0))
        elif todo.all():
            at = d.pos.copy()
            _, out = d.tick()
            for s in range(B):
                assert np.array_equal(out[s], d.want(run, s, at[s])), (g, s)
        else:
            masked_tick(d, b, run, todo)
        g += 1
    assert g == (GROUP_TICKS + 2 if B == 130 else GROUP_TICKS)
    d.close()


def test_groups_of_three_blocks(require_gpu):
    """With the scripts taken cyclically no group of the first 12 ticks holds
    more than 108 of 130 streams.  Here 130 streams play scripts 1, 2 and 3
    (no loss before tick 2, no FEC) and each waits at its first lost tick
    until all stand there: the DC removal of ticks 0 and 1 and the
    concealment of that common tick (the classes differ in the deferred
    frames they flush and meet again at the ring push: the DC add-back and the
    attenuation are one group each) run on 130 streams, three blocks of the
    lane-per-stream kernels with two lanes in the last."""
    run, B = "causal_dc", 130
    scripts = [(1, 2, 3)[s % 3] for s in range(B)]
    b = TG.open_batch(B, run)
    d = TG.Driver(b, scripts, True)
    lost = d.fx["lost"]
    sizes = []
    while True:
        waiting = np.array([bool(lost[scripts[s], d.pos[s]]) for s in range(B)])
        if waiting.all():
            break
        sizes.append(int((~waiting).sum()))
        masked_tick(d, b, run, ~waiting)
    assert sizes[:2] == [B, B] and sorted(set(d.pos)) == [2, 3, 4]
    assert all(b.conceal_state(s)["loss_count"] == 0 for s in (0, 64, 128, 129))
    for _ in range(3):  # the common lost tick, then two more of every stream
        masked_tick(d, b, run, np.ones(B, bool))
    d.close()


# -- 4. a reset in the middle of a burst at FEATURES_DELAY 4 -----------------------------------------------

def test_reset_mid_burst_at_delay_4(require_gpu):
    run, s0 = "d_causal_dc_4", 4  # script 4: ticks 4 .. 15 are lost
    b = open_batch(NS, run)
    d = play(b, run, range(NS), False, ticks=7)
    st = b.conceal_state(s0)
    assert st["loss_count"] == 3 and st["pcm_fill"] == 0 and st["pcm"].size == 880
    b.conceal_reset(s0)
    d.restart(s0)
    st = b.conceal_state(s0)
    assert st["pcm_fill"] == CR.plc_buf_size(4) == 720 and st["loss_count"] == 0 and not st["pcm"].any()
    assert st["dc_mem"] == 0 and st["syn_dc"] == 0
    for t in range(8):
        _, out = d.tick()
        for s in range(NS):
            assert np.array_equal(out[s], d.want(s, t if s == s0 else t + 7)), (t, s)
    d.close()
