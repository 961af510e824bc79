"""The concealment machine (lpcnet_batch_conceal_*) against the fixture
tests/golden/conceal.npz, which tests/conceal_ref.py computes on the CPU:
six streams, each on its own script of lost and received ticks, bit-equal in
the PCM of every tick and in every state the machine touches; the same
streams in a larger batch, under an active mask, after a reset, with FEC,
under another sample kernel; and the calls the machine refuses."""
import numpy as np
import pytest

import conceal_ref as CR
import lpcnet_amd as L

pytestmark = pytest.mark.gpu

NS = len(CR.SCRIPTS)
RUN = {r[0]: r for r in CR.RUNS}
_rows = {}


def fec_row(k):
    if k not in _rows:
        _rows[k] = CR.fec_row(k)
    return _rows[k]


def open_batch(B, run="causal"):
    _, options, delay = RUN[run]
    b = L.LPCNetBatch(B, 0, CR.model_blob(run))
    if delay != 2:
        b.set_model_constants(1.0, delay, False)
    b.conceal_open(options)
    return b


class Driver:
    """Stream s of the batch plays script scripts[s], each stream at its own
    position: the FEC events before a tick, then the tick.  fx: another
    table of the fixture's shape (lost, fec_events, pcm_in and `run`_pcm, a
    row per script); rows(script, k): the k-th FEC frame a script adds."""

    def __init__(self, b, scripts, device, fx=None, rows=None):
        self.b, self.scripts, self.device = b, list(scripts), device
        self.pos = np.zeros(b.B, int)
        self.nfec = np.zeros(b.B, int)
        self.fx = CR.fixture() if fx is None else fx
        self.rows = (lambda sc, k: fec_row(k)) if rows is None else rows
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
                b.conceal_fec_add(s, self.rows(sc, self.nfec[s]))
                self.nfec[s] += 1
            lost[s] = fx["lost"][sc, t]
            pcm[s] = fx["pcm_in"][sc, t]
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

    def want(self, run, s, t):
        return self.fx[f"{run}_pcm"][self.scripts[s], t]

    def close(self):
        if self.d_pcm:
            self.b.device_free(self.d_pcm)
        self.b.close()


def snapshots(b, s):
    """Every state of stream s the machine touches, as comparable bytes."""
    st = b.conceal_state(s)
    return (b.save_state(s), b.plc_save_state(s), b.features_save_state(s), tuple(st[k] for k in CR.CTRL),
            st["features"].tobytes(), st["pcm"].tobytes(), np.float64(st["dc_mem"]).tobytes(), np.float64(st["syn_dc"]).tobytes())


def check_final_state(b, run, s, sc):
    fx = CR.fixture()
    st = b.conceal_state(s)
    assert [st[k] for k in CR.CTRL] == fx[f"{run}_ctrl"][sc].tolist(), (s, "control fields")
    assert st["features"].tobytes() == fx[f"{run}_features"][sc].tobytes(), (s, "st->features")
    assert np.array_equal(st["pcm"], fx[f"{run}_buf"][sc]), (s, "st->pcm")
    assert np.array([st["dc_mem"], st["syn_dc"]]).tobytes() == fx[f"{run}_dc"][sc].tobytes(), (s, "dc_mem / syn_dc")
    g = b.get_state(s)
    assert g["gru_a_state"].tobytes() == fx[f"{run}_gru_a"][sc].tobytes(), (s, "GRU_A state")
    assert g["gru_b_state"].tobytes() == fx[f"{run}_gru_b"][sc].tobytes(), (s, "GRU_B state")
    assert g["frame_count"] == fx[f"{run}_frame_count"][sc], (s, "frame_count")
    assert b.plc_save_state(s) == fx[f"{run}_plc"][sc].tobytes(), (s, "predictor state")
    assert b.features_save_state(s) == fx[f"{run}_enc"][sc].tobytes(), (s, "analysis state")


# -- 1. the six scripts ----------------------------------------------------------------------------

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("run", ["causal", "codec", "causal_dc", "causal_d0", "causal_plc"])
def test_scripts_against_fixture(require_gpu, run, device):
    b = open_batch(NS, run)
    d = Driver(b, range(NS), device)
    for t in range(CR.NTICKS):
        _, out = d.tick()
        for s in range(NS):
            assert np.array_equal(out[s], d.want(run, s, t)), (run, "tick", t, "stream", s, "lost" if d.fx["lost"][s, t] else "received")
    for s in range(NS):
        check_final_state(b, run, s, s)
    d.close()


# -- 2. a stream's result does not depend on who shares its groups --------------------------------------

def test_independence_of_grouping(require_gpu):
    """19 streams, the six scripts cyclically: script 0 four times, the others
    three times, so the groups of a tick (unions of the scripts that make the
    same call) hold 3 to 19 streams and cross the frame kernel's 4-stream
    workgroups and the predictor's 16-stream tile."""
    B = 19
    b = open_batch(B)
    d = Driver(b, [s % NS for s in range(B)], True)
    for t in range(CR.NTICKS):
        _, out = d.tick()
        for s in range(B):
            assert np.array_equal(out[s], d.want("causal", s, t)), (t, s)
    for s in (0, 5, 12, 17, 18):
        check_final_state(b, "causal", s, s % NS)
    d.close()


def test_small_groups(require_gpu):
    """Two streams on scripts 4 and 5, hardly ever in the same state: most groups are one stream."""
    b = open_batch(2, "codec")
    d = Driver(b, [4, 5], False)
    for t in range(16):
        _, out = d.tick()
        for s in range(2):
            assert np.array_equal(out[s], d.want("codec", s, t)), (t, s)
    d.close()


# -- 3. the tick without a loss --------------------------------------------------------------------------

def test_no_loss_tick_launches_no_synthesis(require_gpu):
    b = open_batch(NS)
    twin = L.LPCNetBatch(NS, 0, CR.model_blob("causal"))
    fx = CR.fixture()
    b.reset_timers(2)
    feats = None
    for t in range(5):
        pcm = np.ascontiguousarray(fx["pcm_in"][:, t])
        out = b.conceal_frame(pcm, np.zeros(NS, np.uint8))
        assert np.array_equal(out, pcm)
        feats = twin.plc_update(pcm)
    assert b.kernel_ms(0)[1] == 0 and b.kernel_ms(1)[1] == 0, "a tick without a loss ran a synthesis kernel"
    assert b.kernel_ms(2)[1] == 5 and b.kernel_ms(3)[1] == 5 and b.kernel_ms(6)[1] == 5  # one launch each per tick
    for s in range(NS):
        assert b.conceal_state(s)["features"].tobytes() == feats[s].tobytes(), s
        assert b.plc_save_state(s) == twin.plc_save_state(s) and b.features_save_state(s) == twin.features_save_state(s)
    twin.close()
    b.close()


# -- 4. the active mask ----------------------------------------------------------------------------------

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_active_mask(require_gpu, device):
    b = open_batch(NS)
    d = Driver(b, range(NS), device)
    for t in range(4):
        d.tick()
    idle = [1, 4]  # script 1 is about to lose its first packet, script 4 is inside its burst
    active = np.ones(NS, bool)
    active[idle] = False
    before = [snapshots(b, s) for s in idle]
    for t in range(4, 7):
        given, out = d.tick(active)
        for s in range(NS):
            if s in idle:
                assert np.array_equal(out[s], given[s]), "the row of an inactive stream changed"
            else:
                assert np.array_equal(out[s], d.want("causal", s, t)), (t, s)
    assert [snapshots(b, s) for s in idle] == before, "the state of an inactive stream changed"
    # the idle streams go on from where they stopped
    for t in range(4, 10):
        _, out = d.tick(~active)
        for s in idle:
            assert np.array_equal(out[s], d.want("causal", s, t)), (t, s)
    d.close()


# -- 5. resets -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["conceal_reset", "reset_stream"])
def test_reset_mid_run(require_gpu, how):
    b = open_batch(NS, "causal_dc")
    d = Driver(b, range(NS), False)
    for t in range(7):
        d.tick()
    s0 = 5  # the FEC script, in the middle of its burst with frames queued
    assert b.conceal_state(s0)["fec_fill_pos"] > 0
    if how == "conceal_reset":
        b.conceal_reset(s0)
    else:
        b.reset(s0)
    d.restart(s0)
    assert b.conceal_state(s0)["pcm_fill"] == CR.plc_buf_size(2) and b.conceal_state(s0)["fec_fill_pos"] == 0
    for t in range(8):
        _, out = d.tick()
        for s in range(NS):
            assert np.array_equal(out[s], d.want("causal_dc", s, t if s == s0 else t + 7)), (t, s)
    # every stream at once
    b.conceal_reset()
    for s in range(NS):
        d.restart(s)
    for t in range(3):
        _, out = d.tick()
        for s in range(NS):
            assert np.array_equal(out[s], d.want("causal_dc", s, t)), (t, s)
    d.close()


# -- 6. the FEC queue ------------------------------------------------------------------------------------

def test_fec_buffer_full(require_gpu):
    b = open_batch(2)
    for k in range(100):
        b.conceal_fec_add(1, fec_row(k % 7))
    before = snapshots(b, 1)
    with pytest.raises(L.LPCNetError, match="FEC buffer full"):
        b.conceal_fec_add(1, fec_row(0))
    assert snapshots(b, 1) == before and b.conceal_state(1)["fec_fill_pos"] == 100
    assert b.conceal_state(0)["fec_fill_pos"] == 0
    b.conceal_fec_add(1, None)  # a NULL add only counts
    assert b.conceal_state(1)["fec_skip"] == 1
    b.conceal_fec_clear(1)
    assert [b.conceal_state(1)[k] for k in ("fec_fill_pos", "fec_read_pos", "fec_keep_pos", "fec_skip")] == [0] * 4
    b.close()


def test_fec_compaction(require_gpu):
    """100 frames queued, a burst reads some of them, then an add compacts the
    queue (lpcnet_plc.c:121-124): the frames read next are the right ones."""
    fx = CR.fixture()
    b = open_batch(1, "codec")
    for t in range(CR.COMPACT_TICKS):
        if t == CR.COMPACT_ADD_AT:
            assert b.conceal_state(0)["fec_keep_pos"] > 0 and b.conceal_state(0)["fec_fill_pos"] == 100
        for row in CR.compaction_adds(t):
            b.conceal_fec_add(0, row)
        if t == CR.COMPACT_ADD_AT:
            assert b.conceal_state(0)["fec_keep_pos"] == 0 and b.conceal_state(0)["fec_fill_pos"] < 100
        out = b.conceal_frame(fx["pcm_in"][0, t][None], [CR.COMPACT_LOST[t]])
        assert np.array_equal(out[0], fx["compact_pcm"][t]), t
    st = b.conceal_state(0)
    assert [st[k] for k in CR.CTRL] == fx["compact_ctrl"].tolist()
    assert st["features"].tobytes() == fx["compact_features"].tobytes()
    b.close()


# -- 7. refusals -----------------------------------------------------------------------------------------

def test_arguments(require_gpu):
    lib = L.lib
    pcm = np.zeros((2, 160), np.int16)
    lost = np.zeros(2, np.uint8)
    buf = np.zeros(1024, np.float64)

    def refused(rc, why):
        assert rc == -1 and why in L.last_error(), (rc, L.last_error())

    plain = L.LPCNetBatch(2, 0, L.synthetic_model(1, L.VARIANT_INT8))
    fp32 = L.LPCNetBatch(2, 0, L.synthetic_model(1, L.VARIANT_FP32, plc=True))
    b = L.LPCNetBatch(2, 0, CR.model_blob("causal"))
    empty = L.LPCNetBatch(2, 0)
    for x in (plain, fp32, b, empty):
        x.reset_timers(2)
    refused(lib.lpcnet_batch_conceal_open(None, 0), "null batch")
    refused(lib.lpcnet_batch_conceal_open(empty._b, 0), "no model")
    refused(lib.lpcnet_batch_conceal_open(plain._b, 0), "PLC")
    refused(lib.lpcnet_batch_conceal_open(fp32._b, 0), "PLC")
    refused(lib.lpcnet_batch_conceal_open(b._b, CR.NONCAUSAL), "non-causal")
    refused(lib.lpcnet_batch_conceal_open(b._b, CR.NONCAUSAL | CR.DC_FILTER), "non-causal")
    refused(lib.lpcnet_batch_conceal_open(b._b, 3), "options")
    refused(lib.lpcnet_batch_conceal_open(b._b, 8), "options")
    # no machine open
    d_pcm = b.device_alloc(pcm.nbytes)
    for rc in (lib.lpcnet_batch_conceal_close(b._b), lib.lpcnet_batch_conceal_reset(b._b, 0),
               lib.lpcnet_batch_conceal_frame(b._b, pcm.ctypes.data, lost.ctypes.data, None),
               lib.lpcnet_batch_conceal_frame_device(b._b, d_pcm, lost.ctypes.data, None),
               lib.lpcnet_batch_conceal_fec_add(b._b, 0, None), lib.lpcnet_batch_conceal_fec_clear(b._b, 0),
               lib.lpcnet_batch_conceal_get_state(b._b, 0, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data)):
        refused(rc, "no machine open")
    refused(lib.lpcnet_batch_conceal_frame(None, pcm.ctypes.data, lost.ctypes.data, None), "null batch")
    b.conceal_open(CR.CAUSAL)
    refused(lib.lpcnet_batch_conceal_open(b._b, CR.CAUSAL), "already open")
    refused(lib.lpcnet_batch_conceal_frame(b._b, None, lost.ctypes.data, None), "bad arguments")
    refused(lib.lpcnet_batch_conceal_frame(b._b, pcm.ctypes.data, None, None), "bad arguments")
    refused(lib.lpcnet_batch_conceal_frame_device(b._b, None, lost.ctypes.data, None), "bad arguments")
    refused(lib.lpcnet_batch_conceal_frame_device(b._b, d_pcm, None, None), "bad arguments")
    for s in (-1, 2):
        refused(lib.lpcnet_batch_conceal_fec_add(b._b, s, buf.ctypes.data), "no such stream")
        refused(lib.lpcnet_batch_conceal_fec_clear(b._b, s), "no such stream")
        refused(lib.lpcnet_batch_conceal_get_state(b._b, s, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data),
                "no such stream")
    refused(lib.lpcnet_batch_conceal_reset(b._b, 2), "no such stream")
    refused(lib.lpcnet_batch_conceal_reset(b._b, -2), "no such stream")
    refused(lib.lpcnet_batch_conceal_get_state(b._b, 0, None, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data), "bad arguments")
    # FEATURES_DELAY moved under an open machine
    b.set_model_constants(1.0, 3, False)
    refused(lib.lpcnet_batch_conceal_frame(b._b, pcm.ctypes.data, lost.ctypes.data, None), "FEATURES_DELAY")
    b.set_model_constants(1.0, 2, False)
    for x in (plain, fp32, b, empty):
        x.sync()
        assert [x.kernel_ms(w)[1] for w in range(7)] == [0] * 7, "a refused call launched a timed kernel"
    assert not pcm.any()
    # the machine still works, and a model load closes it
    out = b.conceal_frame(CR.fixture()["pcm_in"][:2, 0], lost)
    assert np.array_equal(out, CR.fixture()["causal_pcm"][:2, 0])
    b.load_model(CR.model_blob("causal"))
    refused(lib.lpcnet_batch_conceal_frame(b._b, pcm.ctypes.data, lost.ctypes.data, None), "no machine open")
    b.conceal_open(CR.CODEC)
    b.conceal_close()
    b.device_free(d_pcm)
    for x in (plain, fp32, b, empty):
        x.close()


# -- 8. the sample kernel does not matter ----------------------------------------------------------------

def test_kernel_choice_does_not_matter(require_gpu):
    outs = []
    for mode in (0, 1):
        b = L.LPCNetBatch(2, 0, CR.model_blob("causal"))
        b.set_kernel(mode)
        b.conceal_open(CR.CAUSAL)
        d = Driver(b, [1, 5], True)
        outs.append(np.stack([d.tick()[1] for _ in range(12)]))
        d.close()
    assert np.array_equal(outs[0], outs[1])
    fx = CR.fixture()
    assert np.array_equal(outs[0][:, 0], fx["causal_pcm"][1, :12]) and np.array_equal(outs[0][:, 1], fx["causal_pcm"][5, :12])


# -- 9. steps on work states leave the batch's frame-count bound alone -----------------------------------

def test_work_state_steps_keep_frame_count_bound(require_gpu):
    """129 streams, the smallest batch on the chunked multi-frame path.  Five
    of them lose packets in the first four ticks, so their synthesis runs on
    the machine's work states and their frame_count advances; the others only
    receive and stay at frame_count 0.  A synthesize_frames call of 8 frames
    must then still start its multi-frame sample launch after the first
    FEATURES_DELAY frames: a bound advanced by the work-state frames gives the
    STATUS_ACTIVITY abort or other PCM than the per-frame path."""
    import test_kernel_choice as KC
    B, F = KC.OVERLAP_MAX_STREAMS + 1, 8
    blob = CR.model_blob("causal")
    plan, _, call, _ = KC.choice(L, blob, B, 0, 0, 0, [], [(F, 160, B, 0, 1, 0, 0, 0, 2, 0)])
    assert plan[KC.PLAN.index("base")] in (1, 2, 3), "the model must plan a matrix-core sample kernel"
    assert call[0] == 1 and call[2] == 1, "8 frames at 129 streams must take the chunked multi-frame path"
    scripts = np.zeros(B, int)
    lossy = {3: 4, 64: 2, 65: 4, 127: 2, 128: 4}  # stream: script; 4 loses ticks 0 and 1, 2 loses ticks 2 and 3
    for s, sc in lossy.items():
        scripts[s] = sc
    feats = np.ascontiguousarray(np.stack([L.synthetic_features(s % 7, F)[:, :20] for s in range(B)], axis=1), np.float32)
    outs = []
    for chunking in (True, False):
        b = open_batch(B)
        b.set_frame_chunking(chunking)
        d = Driver(b, scripts, True)
        for _ in range(4):
            d.tick()
        fc = [b.get_state(s)["frame_count"] for s in range(B)]
        assert all(fc[s] > 0 for s in lossy) and not any(fc[s] for s in range(B) if s not in lossy), fc
        d_f, d_p = b.device_alloc(feats.nbytes), b.device_alloc(F * B * 160 * 2)
        b.h2d(d_f, feats)
        b.synthesize_frames(None, d_f, d_p, F, 160)
        b.sync()
        pcm = np.zeros((F, B, 160), np.int16)
        b.d2h(pcm, d_p)
        outs.append(pcm)
        b.device_free(d_f)
        b.device_free(d_p)
        d.close()
    assert outs[0].any()
    assert np.array_equal(outs[0], outs[1])
