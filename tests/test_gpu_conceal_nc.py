"""The concealment machine's non-causal mode (lpcnet_batch_conceal_open with
LPCNET_CONCEAL_NONCAUSAL) against the fixture tests/golden/conceal_noncausal.npz,
which tests/conceal_nc_ref.py computes on the CPU: six streams, each on its
own script of lost and received ticks, bit-equal in the PCM of every tick and
in every state the machine touches; the same streams in a larger batch at
their own script positions, under an active mask and across a reset; under
the lockstep sample kernel; the 80-sample delay; reopening a batch in another
mode; and the calls the mode refuses."""
import numpy as np
import pytest

import conceal_nc_ref as NR
import conceal_ref as CR
import lpcnet_amd as L

pytestmark = pytest.mark.gpu

NS = len(CR.SCRIPTS)
OPTIONS = dict(NR.RUNS)


def open_batch(B, run):
    b = L.LPCNetBatch(B, 0, NR.model_blob())
    b.set_model_constants(1.0, 0, False)
    b.conceal_open(OPTIONS[run])
    return b


class Driver:
    """Stream s of the batch plays script scripts[s] of a run, each stream at
    its own position: the FEC events before a tick, then the tick.  fx:
    another table of the fixture's shape, a row per script."""

    def __init__(self, b, run, scripts, device, fx=None):
        self.b, self.run, self.scripts, self.device = b, run, list(scripts), device
        self.pos = np.zeros(b.B, int)
        self.nfec = np.zeros(b.B, int)
        self.fx = NR.fixture() if fx is None else fx
        self.d_pcm = b.device_alloc(b.B * 320) if device else None

    def restart(self, s):
        self.pos[s] = self.nfec[s] = 0

    def tick(self, active=None):
        """One tick of every active stream: (the PCM given, the PCM after)."""
        b, fx = self.b, self.fx
        act = np.ones(b.B, bool) if active is None else np.asarray(active, bool)
        lost = np.zeros(b.B, np.uint8)
        pcm = np.full((b.B, 160), 12345, np.int16)
        for s in np.flatnonzero(act):
            sc, t = self.scripts[s], self.pos[s]
            ev = int(fx["fec_events"][sc, t])
            if ev == -2:
                b.conceal_fec_clear(s)
            elif ev == -1:
                b.conceal_fec_add(s, None)
            for _ in range(max(0, ev)):
                b.conceal_fec_add(s, CR.fec_row(self.nfec[s] % 4))
                self.nfec[s] += 1
            lost[s] = fx["lost"][sc, t]
            pcm[s] = fx[f"{self.run}_pcm_in"][sc, t]
        if self.device:
            b.h2d(self.d_pcm, pcm)
            b.conceal_frame_device(self.d_pcm, lost, None if active is None else act)
            b.sync()
            out = np.zeros_like(pcm)
            b.d2h(out, self.d_pcm)
        else:
            out = b.conceal_frame(pcm, lost, None if active is None else act)
        self.pos[act] += 1
        return pcm, out

    def want(self, s, t):
        return self.fx[f"{self.run}_pcm"][self.scripts[s], t]

    def close(self):
        if self.d_pcm:
            self.b.device_free(self.d_pcm)
        self.b.close()


def check_final_state(b, run, s, sc):
    fx = NR.fixture()
    st = b.conceal_state(s)
    assert [st[k] for k in CR.CTRL] == fx[f"{run}_ctrl"][sc].tolist(), (s, "control fields")
    assert st["features"].tobytes() == fx[f"{run}_features"][sc].tobytes(), (s, "st->features")
    assert np.array_equal(st["pcm"][:160], fx[f"{run}_buf"][sc]) and not st["pcm"][160:].any(), (s, "st->pcm")
    assert np.array([st["dc_mem"], st["syn_dc"]]).tobytes() == fx[f"{run}_dc"][sc].tobytes(), (s, "dc_mem / syn_dc")
    nc = b.conceal_state_noncausal(s)
    assert nc["queued_update"] == fx[f"{run}_queued_update"][sc], (s, "queued_update")
    assert np.array_equal(nc["queued_samples"], fx[f"{run}_queued_samples"][sc]), (s, "queued_samples")
    assert np.array_equal(nc["dc_buf"], fx[f"{run}_dcbuf"][sc]), (s, "dc_buf")
    g = b.get_state(s)
    assert g["gru_a_state"].tobytes() == fx[f"{run}_gru_a"][sc].tobytes(), (s, "GRU_A state")
    assert g["gru_b_state"].tobytes() == fx[f"{run}_gru_b"][sc].tobytes(), (s, "GRU_B state")
    assert g["frame_count"] == fx[f"{run}_frame_count"][sc], (s, "frame_count")
    assert b.plc_save_state(s) == fx[f"{run}_plc"][sc].tobytes(), (s, "predictor state")
    assert b.features_save_state(s) == fx[f"{run}_enc"][sc].tobytes(), (s, "analysis state")


def play_fixture(b, run, device):
    d = Driver(b, run, range(NS), device)
    for t in range(CR.NTICKS):
        _, out = d.tick()
        for s in range(NS):
            assert np.array_equal(out[s], d.want(s, t)), (run, "tick", t, "stream", s, "lost" if d.fx["lost"][s, t] else "received")
    for s in range(NS):
        check_final_state(b, run, s, s)
    return d


# -- 1. the six scripts ----------------------------------------------------------------------------

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("run", ["noncausal", "noncausal_dc"])
def test_scripts_against_fixture(require_gpu, run, device):
    play_fixture(open_batch(NS, run), run, device).close()


# -- 2. a larger batch: own positions, an active mask, a reset -------------------------------------------

@pytest.mark.parametrize("run", ["noncausal", "noncausal_dc"])
def test_own_positions_active_mask_and_reset(require_gpu, run):
    """11 streams on the six scripts cyclically.  Stream s starts s // 2 ticks
    late and sits out every tick with (tick + s) % 4 == 0, so the streams of
    one script stand at different positions and a stream's queued update waits
    across ticks it takes no part in; stream 7 is reset in the middle of its
    script (straight after the tick that queued an update) and restarted."""
    B, s0 = 11, 7
    b = open_batch(B, run)
    d = Driver(b, run, [s % NS for s in range(B)], True)
    reset_done = False
    g = 0
    while (d.pos < CR.NTICKS).any():
        act = np.array([g >= s // 2 and (g + s) % 4 != 0 and d.pos[s] < CR.NTICKS for s in range(B)])
        g += 1
        if not act.any():
            continue
        at = d.pos.copy()
        given, out = d.tick(act)
        for s in range(B):
            if act[s]:
                assert np.array_equal(out[s], d.want(s, at[s])), (g, s, at[s])
            else:
                assert np.array_equal(out[s], given[s]), "the row of an inactive stream changed"
        if not reset_done and d.pos[s0] == 6:  # script 1: tick 4 lost, tick 5 queued an update
            assert b.conceal_state_noncausal(s0)["queued_update"] == 1
            b.conceal_reset(s0)
            d.restart(s0)
            nc = b.conceal_state_noncausal(s0)
            assert nc["queued_update"] == 0 and not nc["queued_samples"].any() and not nc["dc_buf"].any()
            assert b.conceal_state(s0)["loss_count"] == 0 and not b.conceal_state(s0)["pcm"].any()
            reset_done = True
    assert reset_done and g > CR.NTICKS
    for s in range(B):
        check_final_state(b, run, s, s % NS)
    d.close()


# -- 3. the sample kernel does not matter ----------------------------------------------------------------

def test_lockstep_sample_kernel(require_gpu):
    run = "noncausal_dc"
    b = L.LPCNetBatch(3, 0, NR.model_blob())
    b.set_model_constants(1.0, 0, False)
    b.set_kernel(1)
    b.conceal_open(OPTIONS[run])
    d = Driver(b, run, [2, 3, 5], True)
    for t in range(CR.NTICKS):
        _, out = d.tick()
        for s in range(3):
            assert np.array_equal(out[s], d.want(s, t)), (t, s)
    for s, sc in enumerate((2, 3, 5)):
        check_final_state(b, run, s, sc)
    d.close()


# -- 4. the output is the input, TRAINING_OFFSET late ------------------------------------------------------

@pytest.mark.parametrize("run", ["noncausal", "noncausal_dc"])
def test_delay_identity(require_gpu, run):
    """lpcnet_plc.c:440-448: without a loss tick t gives in[t-1][80:] then
    in[t][:80], zeros standing in for in[-1], whatever the networks compute."""
    pcm_in = np.ascontiguousarray(CR.received_pcm()[[1, 3, 5], :8].transpose(1, 0, 2))  # [8, 3, 160]
    b = open_batch(3, run)
    prev = np.zeros((3, 160), np.int16)
    for t in range(8):
        out = b.conceal_frame(pcm_in[t], np.zeros(3, np.uint8))
        assert np.array_equal(out[:, :80], prev[:, 80:]) and np.array_equal(out[:, 80:], pcm_in[t][:, :80]), t
        prev = pcm_in[t]
    b.close()


# -- 5. one batch, three machines ------------------------------------------------------------------------

def test_reopen_in_another_mode(require_gpu):
    """Non-causal, causal, non-causal on the same batch at FEATURES_DELAY 0:
    every machine starts from lpcnet_plc_reset and reproduces its fixture."""
    b = open_batch(NS, "noncausal_dc")
    d = play_fixture(b, "noncausal_dc", True)
    b.device_free(d.d_pcm)
    b.conceal_close()
    # the causal_d0 run of tests/golden/conceal.npz
    import test_gpu_conceal as TG
    b.conceal_open(CR.CAUSAL)
    with pytest.raises(L.LPCNetError, match="non-causal"):
        b.conceal_state_noncausal(0)
    causal = TG.Driver(b, range(NS), False)
    for t in range(CR.NTICKS):
        _, out = causal.tick()
        for s in range(NS):
            assert np.array_equal(out[s], causal.want("causal_d0", s, t)), ("causal_d0", t, s)
    for s in range(NS):
        TG.check_final_state(b, "causal_d0", s, s)
    b.conceal_close()
    b.conceal_open(OPTIONS["noncausal"])
    play_fixture(b, "noncausal", False).close()


# -- 6. refusals -----------------------------------------------------------------------------------------

def test_refusals(require_gpu):
    lib = L.lib
    pcm = np.zeros((2, 160), np.int16)
    lost = np.zeros(2, np.uint8)
    q = np.zeros(1, np.int32)

    def refused(rc, *why):
        assert rc == -1 and all(w in L.last_error() for w in why), (rc, L.last_error())

    b = L.LPCNetBatch(2, 0, NR.model_blob())
    b.reset_timers(2)
    # FEATURES_DELAY 2, the default
    for options in (CR.NONCAUSAL, CR.NONCAUSAL | CR.DC_FILTER):
        refused(lib.lpcnet_batch_conceal_open(b._b, options), "non-causal", "FEATURES_DELAY")
    refused(lib.lpcnet_batch_conceal_get_state_noncausal(b._b, 0, q.ctypes.data, None, None), "no machine open")
    # the getter on a causal machine
    b.conceal_open(CR.CAUSAL)
    refused(lib.lpcnet_batch_conceal_get_state_noncausal(b._b, 0, q.ctypes.data, None, None), "non-causal")
    b.conceal_close()
    # a tick after FEATURES_DELAY moved away from 0
    b.set_model_constants(1.0, 0, False)
    b.conceal_open(CR.NONCAUSAL)
    refused(lib.lpcnet_batch_conceal_open(b._b, CR.NONCAUSAL), "already open")
    for s in (-1, 2):
        refused(lib.lpcnet_batch_conceal_get_state_noncausal(b._b, s, q.ctypes.data, None, None), "no such stream")
    assert lib.lpcnet_batch_conceal_get_state_noncausal(b._b, 1, None, None, None) == 0  # every pointer may be NULL
    b.set_model_constants(1.0, 1, False)
    refused(lib.lpcnet_batch_conceal_frame(b._b, pcm.ctypes.data, lost.ctypes.data, None), "FEATURES_DELAY")
    b.sync()
    assert [b.kernel_ms(w)[1] for w in range(7)] == [0] * 7, "a refused call launched a timed kernel"
    assert not pcm.any()
    # back at 0 the machine works
    b.set_model_constants(1.0, 0, False)
    fx = NR.fixture()
    out = b.conceal_frame(fx["noncausal_pcm_in"][:2, 0], lost)
    assert np.array_equal(out, fx["noncausal_pcm"][:2, 0])
    b.close()
