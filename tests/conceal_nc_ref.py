"""CPU reference of the PLC's non-causal mode: lpcnet_plc_update_non_causal,
lpcnet_plc_conceal_non_causal, process_queued_update and clear_state
(lpcnet_plc.c:175-181, 342-492, built as the reference ships it, FEATURES_DELAY
0), one stream, restated line by line in the style of tests/conceal_ref.py and
over the same pinned checkers: oracle_lib.Oracle with the constants (1.0, 0, 0)
(synthesis, state copies), enc_ref.EncRef (the single-frame analysis), burg_ref
(burg_cepstral_analysis) and plc_ref.PlcRef (compute_plc_pred).

ConcealNcRef records the primitive calls it makes as (op, a, b) triples in the
vocabulary of lpcnet_amd/csrc/conceal_plan.h; with stub=True it makes no
numeric call and only the trace and the control fields are real, which is what
tests/test_conceal_nc_plan.py compares the planner against.  pcm_save (:373,
:399) is the frame as it stands until :440 and has no step of its own.

Also the loader of the fixture tests/golden/conceal_noncausal.npz
(tests/golden/make_conceal_nc_golden.py writes it).
TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import math
import os

import numpy as np

from conceal_ref import (ANALYSIS, ATT_TABLE, ATTENUATE, BURG, COUNTERS, CP_BURG_ONLY, CP_FULL, CP_ZERO, CTRL, DC_CONCEAL, DC_CONST,
                         DC_FILTER, DC_REMOVE, DC_RESTORE, FRAME_SIZE, IMPL, NB_BANDS, NB_FEATURES, NONCAUSAL, NTICKS,
                         PCM_MOVE, PLC_MAX_FEC, PREDICT, RESET_SIGNAL, SCRIPTS, SIGNALS, TAIL, TRAINING_OFFSET, CM_TAIL_HALF, F,
                         _short, _wraps, fec_events, fec_row, lost_matrix, plc_buf_size, received_pcm)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conceal_noncausal.npz")
HALF = TRAINING_OFFSET

# conceal_plan.h: the steps and parameter values the non-causal mode adds
SYN_SAVE, SYN_RESTORE, DC_REDO, REVERSE, BLEND_BACK, QUEUE_FILL, REORDER = range(20, 27)
OP_NAMES = {20: "SYN_SAVE", 21: "SYN_RESTORE", 22: "DC_REDO", 23: "REVERSE", 24: "BLEND_BACK", 25: "QUEUE_FILL", 26: "REORDER"}
CI_QUEUE, CI_BUF_OUT, CI_REV, CI_ANALYSED, CI_BUF_HI, CI_PCM_LO = range(4, 10)
CT_PCM, CT_REV, CT_PCM_PRE, CT_PCM_HI = range(4)
CM_HEAD_OUT, CM_HEAD_IN = 4, 5
CA_PCM, CA_BUF = 0, 1
CDC_CAUSAL, CDC_NONCAUSAL, CDC_FIRST_LOSS = range(3)
# (name, options) of the fixture's runs, both on the small predictor shape at FEATURES_DELAY 0
RUNS = [("noncausal", NONCAUSAL), ("noncausal_dc", NONCAUSAL | DC_FILTER)]


class ConcealNcRef:
    """One LPCNetPLCState opened with LPCNET_PLC_NONCAUSAL, with or without
    DC_FILTER, on a model built with FEATURES_DELAY 0."""

    def __init__(self, blob: bytes | None = None, options: int = NONCAUSAL, stub: bool = False):
        if options & 3 != NONCAUSAL or options & ~7:
            raise ValueError("the non-causal mode only")
        self.remove_dc = bool(options & DC_FILTER)  # :77
        self.buf = plc_buf_size(0)
        self.stub = stub
        self.trace = []
        self.count = dict.fromkeys(COUNTERS, 0)  # conceal_ref.COUNTERS; the ring and the long moves are not this mode's
        if not stub:
            import burg_ref
            import enc_ref
            import oracle_lib as O
            import plc_ref
            self.lpcnet = O.Oracle(blob, 0, None, (1.0, 0, 0))
            self.enc = enc_ref.EncRef()
            self.net = plc_ref.PlcRef(blob)
            self._burg = burg_ref.ref_frame if burg_ref.have_ref() else burg_ref.burg_frame
            self.lpcnet.reset()
            self._ulaw0 = self.lpcnet.tail()[2]  # lin2ulaw(0.f): last_exc after lpcnet_reset (lpcnet.c:226-233)
        self.reset()

    # -- lpcnet_plc_reset (:46-59) --------------------------------------------
    def reset(self):
        self.fec_keep_pos = self.fec_read_pos = self.fec_fill_pos = self.fec_skip = 0
        self.pcm = np.zeros(self.buf + FRAME_SIZE, np.int16)
        self.features = np.zeros(NB_FEATURES, F)
        self.dc_mem = 0.0
        self.syn_dc = 0.0
        self.dc_buf = np.zeros(TRAINING_OFFSET, np.int16)
        self.queued_samples = np.zeros(FRAME_SIZE, np.int16)
        self.queued_update = 0
        self.pcm_fill = self.buf
        self.skip_analysis = 0
        self.blend = 0
        self.loss_count = 0
        self.feature_buffer_fill = 0
        if not self.stub:
            self.lpcnet.reset()
            self.enc.reset()
            self.net.reset()

    def ctrl(self) -> dict:
        return {k: int(getattr(self, k)) for k in CTRL}

    def _t(self, op, a=0, b=0):
        self.trace.append((op, a, b))

    def take_trace(self) -> list:
        t, self.trace = self.trace, []
        return t

    # -- lpcnet_plc_fec_add / _fec_clear (:111-132): the positions move, the mode never reads the queue
    def fec_add(self, features) -> bool:
        if features is None:
            self.fec_skip += 1
            return True
        if self.fec_fill_pos == PLC_MAX_FEC:
            if self.fec_keep_pos == 0:
                return False
            self.fec_fill_pos -= self.fec_keep_pos
            self.fec_read_pos -= self.fec_keep_pos
            self.fec_keep_pos = 0
        self.fec_fill_pos += 1
        return True

    def fec_clear(self):
        self.fec_keep_pos = self.fec_read_pos = self.fec_fill_pos = self.fec_skip = 0

    # -- the primitive calls ----------------------------------------------------
    def _pred(self, kind, row=None):  # compute_plc_pred (:135-145) into st->features
        self._t(PREDICT, kind)
        if not self.stub:
            self.features = self.net.predict(row)

    def _analysis(self, pcm, what):  # preemphasis, compute_frame_features, process_single_frame
        self._t(ANALYSIS, what)
        return None if self.stub else self.enc.frame(np.array(pcm, np.int16))[:NB_FEATURES]

    def _clear_state(self):  # :175-181
        self._t(RESET_SIGNAL)
        if not self.stub:
            _, _, _, rng = self.lpcnet.tail()
            self.lpcnet.set_tail(np.zeros(16, F), 0.0, self._ulaw0, rng)
            self.lpcnet.set_state(np.zeros(384, F), np.zeros(16, F))

    def _process_queued_update(self):  # :342-347
        if self.queued_update:
            self._t(IMPL, FRAME_SIZE, CI_QUEUE)
            if not self.stub:
                self.lpcnet.synthesize(self.features, FRAME_SIZE, preload=self.queued_samples)
            self.queued_update = 0

    def _dc_pass(self, pcm, lp):  # :367-371, :394-398
        for i in range(FRAME_SIZE):
            lp[i] = _short(math.floor(.5 + self.dc_mem))
            self.count["dc_tie"] += self.dc_mem - math.floor(self.dc_mem) == .5 and math.floor(self.dc_mem) % 2 == 0
            self.dc_mem += DC_CONST * (float(pcm[i]) - self.dc_mem)
            self.count["l_negative"] += lp[i] < 0
            self.count["dc_remove_wrap"] += _wraps(int(pcm[i]) - int(lp[i]))
            pcm[i] = _short(int(pcm[i]) - int(lp[i]))

    def _attenuate(self):  # :460-461
        self._t(ATTENUATE, self.loss_count)
        f0 = self.features[0]
        if self.loss_count >= 10:
            v = F(F(f0 + ATT_TABLE[9]) - F(2 * (self.loss_count - 9)))
        else:
            v = F(f0 + ATT_TABLE[self.loss_count])
        self.count["loss_ge_10"] += self.loss_count >= 10
        self.count["clamp"] += bool(-10 > v)
        self.features[0] = F(-10) if -10 > v else v

    # -- lpcnet_plc_update_non_causal (:349-450) ---------------------------------
    def update(self, pcm_in) -> np.ndarray:
        pcm = np.array(pcm_in, np.int16)
        assert pcm.shape == (FRAME_SIZE,)
        stub = self.stub
        lp = np.zeros(FRAME_SIZE, np.int16)
        mem_bak = 0.0
        delta = int(self.syn_dc)  # :356
        self.count["delta_trunc"] += delta < 0 and delta != math.floor(self.syn_dc)
        self._process_queued_update()  # :362
        if self.remove_dc:  # :363-372
            self._t(DC_REMOVE, CDC_NONCAUSAL)
            self.dc_mem += self.syn_dc
            self.syn_dc = 0.0
            mem_bak = self.dc_mem
            self._dc_pass(pcm, lp)
        pcm_save = pcm.copy()  # :373
        self._t(BURG, 1 if self.loss_count > 0 else 0)
        plc_features = np.zeros(2 * NB_BANDS + NB_FEATURES + 1, F)
        if not stub:
            plc_features[:2 * NB_BANDS] = self._burg(pcm)[0]  # :374-375
        if self.loss_count > 0:
            zeros = np.zeros_like(plc_features)  # :380-382
            zeros[:2 * NB_BANDS] = plc_features[:2 * NB_BANDS]
            zeros[-1] = 1
            self._pred(CP_BURG_ONLY, zeros)  # :383
            self._t(SYN_SAVE)  # :384
            copy = None if stub else self.lpcnet.save()
            self._t(IMPL, TRAINING_OFFSET, CI_BUF_OUT)  # :385
            if not stub:
                self.pcm[HALF:FRAME_SIZE] = self.lpcnet.synthesize(self.features, TRAINING_OFFSET)
            if self.remove_dc:  # :387-400
                self._t(DC_REDO)
                for i in range(FRAME_SIZE):
                    self.count["dc_add_wrap"] += _wraps(int(pcm[i]) + int(lp[i]))
                    pcm[i] = _short(int(pcm[i]) + int(lp[i]))
                self.dc_mem = mem_bak
                for i in range(TRAINING_OFFSET):
                    self.syn_dc += DC_CONST * (float(self.pcm[HALF + i]) - self.syn_dc)
                self.dc_mem += self.syn_dc
                delta = int(float(delta) + self.syn_dc)  # int delta += a double
                self.syn_dc = 0.0
                self._dc_pass(pcm, lp)
                pcm_save = pcm.copy()
            self._t(REVERSE)  # :403
            rev = pcm[::-1].copy()
            self._clear_state()  # :404
            self._t(IMPL, FRAME_SIZE, CI_REV)  # :405
            if not stub:
                self.lpcnet.synthesize(self.features, FRAME_SIZE, preload=rev)
            self._t(TAIL, TRAINING_OFFSET, CT_REV)  # :406
            if not stub:
                rev[:TRAINING_OFFSET] = self.lpcnet.synthesize_tail(np.zeros(TRAINING_OFFSET, np.int16), 0)
            self._t(BLEND_BACK)  # :407-411
            if not stub:
                for i in range(TRAINING_OFFSET):
                    w = F(.5 - .5 * math.cos(math.pi * i / TRAINING_OFFSET))
                    j = FRAME_SIZE - 1 - i
                    a = F(w * F(self.pcm[j]))
                    c = F(F(F(1) - w) * F(int(rev[i]) + delta))
                    self.count["blend_wrap"] += _wraps(math.floor((.5 + float(a)) + float(c)))
                    self.pcm[j] = _short(math.floor((.5 + float(a)) + float(c)))
            self._t(SYN_RESTORE)  # :414
            if not stub:
                self.lpcnet.restore(copy)
            self._t(QUEUE_FILL)  # :416-418
            self.queued_update = 1
            self.queued_samples[:TRAINING_OFFSET] = self.pcm[HALF:FRAME_SIZE]
            self.queued_samples[TRAINING_OFFSET:] = pcm[:HALF]
            self._analysis(self.pcm[:FRAME_SIZE], CA_BUF)  # :423-426
        enc_features = self._analysis(pcm, CA_PCM)  # :429-432
        if self.loss_count == 0:
            if not stub:
                plc_features[2 * NB_BANDS:2 * NB_BANDS + NB_FEATURES] = enc_features  # :434-435
                plc_features[-1] = 1
            self._pred(CP_FULL, plc_features)  # :436
            self._t(IMPL, TRAINING_OFFSET, CI_ANALYSED)  # :437
            if not stub:
                self.lpcnet.synthesize(enc_features, TRAINING_OFFSET, preload=self.pcm[HALF:FRAME_SIZE])
            self._t(TAIL, HALF, CT_PCM_PRE)  # :438
            if not stub:
                self.lpcnet.synthesize_tail(pcm[:HALF], HALF)
        self._t(REORDER)  # :440-442
        pcm[HALF:] = pcm[:TRAINING_OFFSET].copy()
        pcm[:HALF] = self.pcm[TRAINING_OFFSET:FRAME_SIZE]
        self.pcm[:FRAME_SIZE] = pcm_save
        self.loss_count = 0
        if self.remove_dc:  # :444-448
            self._t(DC_RESTORE, CDC_NONCAUSAL)
            for i in range(TRAINING_OFFSET):
                self.count["dc_add_wrap"] += _wraps(int(pcm[i]) + int(self.dc_buf[i]))
                pcm[i] = _short(int(pcm[i]) + int(self.dc_buf[i]))
            for i in range(TRAINING_OFFSET, FRAME_SIZE):
                self.count["dc_add_wrap"] += _wraps(int(pcm[i]) + int(lp[i - TRAINING_OFFSET]))
                pcm[i] = _short(int(pcm[i]) + int(lp[i - TRAINING_OFFSET]))
            self.dc_buf[:] = lp[HALF:]
        return pcm

    # -- lpcnet_plc_conceal_non_causal (:452-492) -----------------------------------
    def conceal(self) -> np.ndarray:
        stub = self.stub
        pcm = np.zeros(FRAME_SIZE, np.int16)
        self._process_queued_update()  # :456
        self._pred(CP_ZERO, None)  # :459
        self._attenuate()  # :460-461
        if self.loss_count == 0:
            self._t(PCM_MOVE, CM_HEAD_OUT)  # :464
            pcm[:TRAINING_OFFSET] = self.pcm[HALF:FRAME_SIZE]
            self._t(IMPL, TRAINING_OFFSET, CI_BUF_HI)  # :465
            if not stub:
                self.lpcnet.synthesize(self.features, TRAINING_OFFSET, preload=self.pcm[HALF:FRAME_SIZE])
            self._t(TAIL, HALF, CT_PCM_HI)  # :466
            if not stub:
                pcm[TRAINING_OFFSET:] = self.lpcnet.synthesize_tail(np.zeros(HALF, np.int16), 0)
        else:
            self._t(IMPL, TRAINING_OFFSET, CI_PCM_LO)  # :468
            if not stub:
                pcm[:TRAINING_OFFSET] = self.lpcnet.synthesize(self.features, TRAINING_OFFSET)
            self._t(TAIL, HALF, CT_PCM_HI)  # :469
            if not stub:
                pcm[TRAINING_OFFSET:] = self.lpcnet.synthesize_tail(np.zeros(HALF, np.int16), 0)
            self._t(PCM_MOVE, CM_HEAD_IN)  # :471
            self.pcm[HALF:FRAME_SIZE] = pcm[:TRAINING_OFFSET]
            self._analysis(self.pcm[:FRAME_SIZE], CA_BUF)  # :472-475
        self._t(PCM_MOVE, CM_TAIL_HALF)  # :477
        self.pcm[:HALF] = pcm[TRAINING_OFFSET:]
        if self.remove_dc:  # :479-489
            self._t(DC_CONCEAL, CDC_FIRST_LOSS if self.loss_count == 0 else CDC_NONCAUSAL)
            dc = int(math.floor(.5 + self.dc_mem))
            self.count["l_negative"] += dc < 0
            for i in range(TRAINING_OFFSET if self.loss_count == 0 else 0, FRAME_SIZE):
                self.syn_dc += DC_CONST * (float(pcm[i]) - self.syn_dc)
            for i in range(TRAINING_OFFSET):
                self.count["dc_add_wrap"] += _wraps(int(pcm[i]) + int(self.dc_buf[i]))
                pcm[i] = _short(int(pcm[i]) + int(self.dc_buf[i]))
            for i in range(TRAINING_OFFSET, FRAME_SIZE):
                self.count["dc_add_wrap"] += _wraps(int(pcm[i]) + dc)
                pcm[i] = _short(int(pcm[i]) + dc)
            self.dc_buf[:] = _short(dc)
        self.loss_count += 1  # :490
        return pcm

    def tick(self, pcm, lost: bool) -> np.ndarray:
        return self.conceal() if lost else self.update(pcm)


# -- the fixture ------------------------------------------------------------------------

def model_blob() -> bytes:
    import lpcnet_amd as L
    return L.synthetic_model(1, L.VARIANT_INT8, codebooks=False, plc=False, plc_small=True)


def burg_frame_ok(p) -> None:
    """A frame that reaches burg_cepstral_analysis must be inside its
    contract (the reference asserts otherwise): fail loudly."""
    import burg_ref
    p = np.array(p, np.int16)
    for h in (p[:HALF], p[HALF:]):
        if not h.any():
            raise ValueError("an all-zero half-frame reaches burg_cepstral_analysis")
    if not np.isfinite(burg_ref.burg_frame(p)[0]).all():
        raise ValueError("burg_cepstral_analysis is not finite on a received frame")


def check_received(ref: ConcealNcRef, pcm) -> None:
    """The frame Burg analyses (:374-375) is the first DC pass (:363-372) of
    the received one, whatever the redo pass makes of it later."""
    p = np.array(pcm, np.int16)
    if ref.remove_dc:
        dc_mem = ref.dc_mem + ref.syn_dc
        for i in range(FRAME_SIZE):
            l = _short(math.floor(.5 + dc_mem))
            dc_mem += DC_CONST * (float(p[i]) - dc_mem)
            p[i] = _short(int(p[i]) - l)
    burg_frame_ok(p)


def signal_pcm(name: str) -> np.ndarray:
    """[28, 160] int16 of one signal of tests/feat_signals.py, as conceal_ref.received_pcm lays it out."""
    import feat_signals as FS
    p = FS.pcm_of(name)
    return p[np.arange(NTICKS) % len(p)]


def run_script(ref: ConcealNcRef, stream: int, pcm: np.ndarray, on_received=None) -> np.ndarray:
    """Script `stream` on ``ref`` from reset: the PCM of every tick [28, 160]."""
    lost, ev = lost_matrix()[stream], fec_events(stream)
    out = np.zeros((NTICKS, FRAME_SIZE), np.int16)
    k = 0
    for t in range(NTICKS):
        if ev[t] == -2:
            ref.fec_clear()
        elif ev[t] == -1:
            ref.fec_add(None)
        for _ in range(max(0, int(ev[t]))):
            ref.fec_add(fec_row(k))
            k += 1
        if on_received is not None and not lost[t]:
            on_received(ref, pcm[t])
        out[t] = ref.tick(pcm[t], bool(lost[t]))
    return out


KEYS = ("pcm", "ctrl", "queued_update", "queued_samples", "dcbuf", "features", "buf", "dc", "gru_a", "gru_b", "frame_count",
        "plc", "enc")


def compute_run(options: int, pcm_in: np.ndarray, streams=None, check: bool = True) -> dict:
    """The arrays of one run of the fixture (keys without the run's prefix); pcm_in [6, 28, 160]."""
    blob = model_blob()
    streams = range(len(SCRIPTS)) if streams is None else streams
    out = {k: [] for k in KEYS}
    for s in streams:
        ref = ConcealNcRef(blob, options)
        out["pcm"].append(run_script(ref, s, pcm_in[s], check_received if check else None))
        c = ref.ctrl()
        out["ctrl"].append(np.array([c[k] for k in CTRL], np.int32))
        out["queued_update"].append(np.int32(ref.queued_update))
        out["queued_samples"].append(ref.queued_samples.copy())
        out["dcbuf"].append(ref.dc_buf.copy())
        out["features"].append(ref.features.copy())
        out["buf"].append(ref.pcm[:FRAME_SIZE].copy())
        out["dc"].append(np.array([ref.dc_mem, ref.syn_dc], np.float64))
        a, b = ref.lpcnet.state()
        out["gru_a"].append(a)
        out["gru_b"].append(b)
        out["frame_count"].append(np.int32(ref.lpcnet.frame_count()))
        out["plc"].append(np.frombuffer(ref.net.save(), F).copy())
        out["enc"].append(np.frombuffer(ref.enc.state_bytes(), np.uint8).copy())
    return {k: np.stack(v) for k, v in out.items()}


_fix = None


def fixture() -> dict:
    """The committed fixture, read-only.  signals [6] (names of
    tests/feat_signals.py, per run r: r_signals), r_pcm_in [6, 28, 160]; per
    run r of RUNS: r_pcm [6, 28, 160], r_ctrl [6, 9], r_queued_update [6],
    r_queued_samples [6, 160], r_dcbuf [6, 80] (dc_buf), r_features [6, 20], r_buf
    [6, 160] (st->pcm[0 .. 160)), r_dc [6, 2] float64, r_gru_a [6, 384],
    r_gru_b [6, 16], r_frame_count [6], r_plc [6, n1 + n2] float32 and r_enc
    [6, state bytes] uint8."""
    global _fix
    if _fix is None:
        with np.load(GOLDEN) as g:
            _fix = {k: g[k] for k in g.files}
        for v in _fix.values():
            v.setflags(write=False)
    return _fix
