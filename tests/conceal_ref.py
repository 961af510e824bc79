"""CPU reference of the PLC's state machine: lpcnet_plc_update_causal /
lpcnet_plc_conceal_causal with lpcnet_plc_reset, lpcnet_plc_fec_add / _clear,
get_fec_or_pred and fec_rewind (lpcnet_plc.c:46-59, 111-132, 147-173, 188-337,
built as the reference ships it, PLC_SKIP_UPDATES defined), one stream.  The
glue is restated here line by line; every network and analysis call goes to
a checker that is pinned to the reference's own compiled kernels elsewhere:
oracle_lib.Oracle (synthesis, deferred frames, reset_signal, state copies),
enc_ref.EncRef (the single-frame analysis), burg_ref (burg_cepstral_analysis)
and plc_ref.PlcRef (compute_plc_pred).  lpcnet_plc.c itself cannot be compiled
from the reference tree (it includes the generated plc_data.h / nnet_data.h).

ConcealRef records the primitive calls it makes as (op, a, b) triples in the
vocabulary of lpcnet_amd/csrc/conceal_plan.h; with stub=True it makes no
numeric call at all and only the trace and the control fields are real, which
is what tests/test_conceal_plan.py compares the planner against.

Also the loss and FEC scripts, signals and loader of the fixture
tests/golden/conceal.npz (tests/golden/make_conceal_golden.py writes it).
TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import math
import os

import numpy as np

F = np.float32
FRAME_SIZE = 160
TRAINING_OFFSET = 80
HALF = FRAME_SIZE - TRAINING_OFFSET
NB_BANDS = 18
NB_FEATURES = 20
PLC_MAX_FEC = 100           # lpcnet_private.h:25
MAX_FEATURE_BUFFER = 4      # lpcnet_private.h:26; conv1 + conv2 kernel sizes - 2 of the default model
DC_CONST = 0.003            # lpcnet_plc.c:183
ATT_TABLE = [F(v) for v in (0, 0, -.2, -.2, -.4, -.4, -.8, -.8, -1.6, -1.6)]  # :292
CAUSAL, NONCAUSAL, CODEC, DC_FILTER = 0, 1, 2, 4  # include/lpcnet.h LPCNET_PLC_*
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conceal.npz")

# conceal_plan.h: enum ConcealOp and its parameter values
(DC_REMOVE, DC_RESTORE, DC_CONCEAL, BURG, ANALYSIS, PREDICT, PLC_PUSH, PLC_RESTORE, FEC_FETCH, DEFER_PUSH, FLUSH, IMPL,
 TAIL, RESET_SIGNAL, BLEND, ATTENUATE, PCM_MOVE, FEC_REWIND, FEC_DISCARD) = range(1, 20)
OP_NAMES = ["", "DC_REMOVE", "DC_RESTORE", "DC_CONCEAL", "BURG", "ANALYSIS", "PREDICT", "PLC_PUSH", "PLC_RESTORE", "FEC_FETCH",
            "DEFER_PUSH", "FLUSH", "IMPL", "TAIL", "RESET_SIGNAL", "BLEND", "ATTENUATE", "PCM_MOVE", "FEC_REWIND", "FEC_DISCARD"]
CP_FULL, CP_BURG_ONLY, CP_ROW_DISCARD, CP_ZERO = range(4)
CD_FEATURES, CD_ANALYSED = range(2)
CI_BUF, CI_SPEC, CI_PCM_PRE, CI_PCM_OUT = range(4)
CM_TAIL_HALF, CM_APPEND, CM_NEWEST, CM_SHIFT = range(4)
CTRL = ("pcm_fill", "skip_analysis", "blend", "loss_count", "fec_fill_pos", "fec_read_pos", "fec_keep_pos", "fec_skip",
        "feature_buffer_fill")


def plc_buf_size(delay: int) -> int:
    return delay * FRAME_SIZE + TRAINING_OFFSET  # lpcnet_private.h:77


def _short(v: int) -> int:
    """An int stored into a short (x86: modulo 2^16)."""
    return ((int(v) + 32768) & 0xFFFF) - 32768


# What a run went through, counted beside the arithmetic (tests/test_conceal_edge_ref.py reads the aims of
# tests/conceal_edge.py's cases from them); no counter feeds back into a value.
COUNTERS = ("dc_remove_wrap",   # pcm - l left int16 before its short store (:202)
            "dc_add_wrap",      # pcm + lp (:285) or pcm + add (:333) did
            "l_negative",       # floor(.5 + dc_mem) < 0
            "delta_trunc",      # delta < 0 and (int)syn_dc != floor(syn_dc)
            "blend_wrap",       # the blend's integer left int16 before its short store (:228, :411)
            "clamp",            # MAX16(-10, .) took the -10 (:319)
            "loss_ge_10",       # the loss_count >= 10 branch of :319
            "move_max",         # the longest PCM_MOVE, in shorts
            "restore_at_delay",  # PLC_RESTORE with which == FEATURES_DELAY (:217)
            "dc_tie")           # floor(.5 + dc_mem) on a dc_mem of an even integer + .5 exactly, where rint goes down


def _wraps(v: int) -> bool:
    return not -32768 <= int(v) <= 32767


class ConcealRef:
    """One LPCNetPLCState.  options: CAUSAL or CODEC, with or without
    DC_FILTER; delay: FEATURES_DELAY of the model's build."""

    def __init__(self, blob: bytes | None = None, options: int = CAUSAL, delay: int = 2, stub: bool = False):
        mode = options & 3
        if mode not in (CAUSAL, CODEC):
            raise ValueError("the causal and codec modes only")
        self.enable_blending = mode == CAUSAL  # :65-73
        self.remove_dc = bool(options & DC_FILTER)  # :77
        self.delay = delay
        self.buf = plc_buf_size(delay)
        self.stub = stub
        self.trace = []
        self.count = dict.fromkeys(COUNTERS, 0)
        if not stub:
            import burg_ref
            import enc_ref
            import oracle_lib as O
            import plc_ref
            self.lpcnet = O.Oracle(blob, 0, None, (1.0, delay, 0))
            self.enc = enc_ref.EncRef()
            self.net = plc_ref.PlcRef(blob)
            self._burg = burg_ref.ref_frame if burg_ref.have_ref() else burg_ref.burg_frame
        self.reset()

    # -- lpcnet_plc_reset (:46-59) --------------------------------------------
    def reset(self):
        self.fec = np.zeros((PLC_MAX_FEC, NB_FEATURES), F)
        self.fec_keep_pos = self.fec_read_pos = self.fec_fill_pos = self.fec_skip = 0
        self.pcm = np.zeros(self.buf + FRAME_SIZE, np.int16)
        self.features = np.zeros(NB_FEATURES, F)
        self.dc_mem = 0.0
        self.syn_dc = 0.0
        self.pcm_fill = self.buf
        self.skip_analysis = 0
        self.blend = 0
        self.loss_count = 0
        self.feature_buffer_fill = 0  # the LPCNetState's, cleared by lpcnet_reset
        if not self.stub:
            self.lpcnet.reset()
            self.enc.reset()
            self.net.reset()
            self.plc_copy = [self.net.save() for _ in range(self.delay + 1)]

    def ctrl(self) -> dict:
        return {k: int(getattr(self, k)) for k in CTRL}

    def _t(self, op, a=0, b=0):
        self.trace.append((op, a, b))

    # -- lpcnet_plc_fec_add / _fec_clear (:111-132) -----------------------------
    def fec_add(self, features) -> bool:
        """False: "FEC buffer full", nothing changed."""
        if features is None:
            self.fec_skip += 1
            return True
        if self.fec_fill_pos == PLC_MAX_FEC:
            if self.fec_keep_pos == 0:
                return False
            n = self.fec_fill_pos - self.fec_keep_pos
            self.fec[:n] = self.fec[self.fec_keep_pos:self.fec_fill_pos].copy()
            self.fec_fill_pos -= self.fec_keep_pos
            self.fec_read_pos -= self.fec_keep_pos
            self.fec_keep_pos = 0
        self.fec[self.fec_fill_pos] = np.asarray(features, F)[:NB_FEATURES]
        self.fec_fill_pos += 1
        return True

    def fec_clear(self):
        self.fec_keep_pos = self.fec_read_pos = self.fec_fill_pos = self.fec_skip = 0

    # -- the primitive calls ----------------------------------------------------
    def _pred(self, kind, row=None, keep=True):
        """compute_plc_pred (:135-145) into st->features, or discarded."""
        self._t(PREDICT, kind)
        if not self.stub:
            out = self.net.predict(row)
            if keep:
                self.features = out

    def _keep_pos(self):
        self.fec_keep_pos = max(0, max(self.fec_keep_pos, self.fec_read_pos - self.delay - 1))

    def _get_fec_or_pred(self) -> int:  # :147-166
        if self.fec_read_pos != self.fec_fill_pos and self.fec_skip == 0:
            self._t(FEC_FETCH, self.fec_read_pos)
            self.features = self.fec[self.fec_read_pos].copy()
            row = np.zeros(2 * NB_BANDS + NB_FEATURES + 1, F)
            self.fec_read_pos += 1
            self._keep_pos()
            row[2 * NB_BANDS:2 * NB_BANDS + NB_FEATURES] = self.features
            row[-1] = -1
            self._pred(CP_ROW_DISCARD, row, keep=False)
            return 1
        self._pred(CP_ZERO, None)
        if self.fec_skip > 0:
            self.fec_skip -= 1
        return 0

    def _deferred(self, what, feats):  # run_frame_network_deferred (lpcnet.c:122-132)
        self._t(DEFER_PUSH, what, self.feature_buffer_fill)
        if self.feature_buffer_fill < MAX_FEATURE_BUFFER:
            self.feature_buffer_fill += 1
        if not self.stub:
            self.lpcnet.frame_deferred(feats)

    def _plc_push(self):  # :305-306, :313-314
        self._t(PLC_PUSH)
        if not self.stub:
            self.plc_copy = [self.net.save()] + self.plc_copy[:self.delay]

    def _plc_restore(self, k):
        self._t(PLC_RESTORE, k)
        self.count["restore_at_delay"] += k == self.delay
        if not self.stub:
            self.net.restore(self.plc_copy[k])

    def _analysis(self, pcm):  # :251-254, :322-328
        self._t(ANALYSIS)
        return None if self.stub else self.enc.frame(pcm)[:NB_FEATURES]

    def _moved(self, n):
        self.count["move_max"] = max(self.count["move_max"], n)

    def _shift(self):
        self._t(PCM_MOVE, CM_SHIFT)
        self._moved(self.buf)
        self.pcm[:self.buf] = self.pcm[FRAME_SIZE:FRAME_SIZE + self.buf].copy()  # RNN_MOVE

    # -- lpcnet_plc_update_causal (:188-290) --------------------------------------
    def update(self, pcm_in) -> np.ndarray:
        pcm = np.array(pcm_in, np.int16)
        assert pcm.shape == (FRAME_SIZE,)
        stub = self.stub
        lp = np.zeros(FRAME_SIZE, np.int16)
        delta = 0
        if self.remove_dc:  # :195-204
            self._t(DC_REMOVE)
            self.dc_mem += self.syn_dc
            delta = int(self.syn_dc)
            self.count["delta_trunc"] += delta < 0 and delta != math.floor(self.syn_dc)
            self.syn_dc = 0.0
            for i in range(FRAME_SIZE):
                lp[i] = _short(math.floor(.5 + self.dc_mem))
                self.count["dc_tie"] += self.dc_mem - math.floor(self.dc_mem) == .5 and math.floor(self.dc_mem) % 2 == 0
                self.dc_mem += DC_CONST * (float(pcm[i]) - self.dc_mem)
                self.count["l_negative"] += lp[i] < 0
                self.count["dc_remove_wrap"] += _wraps(int(pcm[i]) - int(lp[i]))
                pcm[i] = _short(int(pcm[i]) - int(lp[i]))
        blend_now = bool(self.skip_analysis and self.blend and self.enable_blending)
        self._t(BURG, 1 if blend_now else 0)
        plc_features = np.zeros(2 * NB_BANDS + NB_FEATURES + 1, F)
        if not stub:
            plc_features[:2 * NB_BANDS] = self._burg(pcm)[0]  # :205-206
        if self.skip_analysis:
            if self.blend:
                if self.enable_blending:
                    zeros = np.zeros_like(plc_features)  # :212-214
                    zeros[:2 * NB_BANDS] = plc_features[:2 * NB_BANDS]
                    zeros[-1] = 1
                    self._plc_restore(self.delay)  # :217
                    self._pred(CP_BURG_ONLY, zeros)  # :218
                    for _ in range(self.delay):  # :219-222
                        self._deferred(CD_FEATURES, self.features)
                    self._t(IMPL, HALF, CI_SPEC)  # :223-224, :230
                    if not stub:
                        copy = self.lpcnet.save()
                        tmp = self.lpcnet.synthesize(self.features, HALF)
                        self.lpcnet.restore(copy)
                    self._t(BLEND)  # :225-229
                    if not stub:
                        for i in range(HALF):
                            w = F(.5 - .5 * math.cos(math.pi * i / HALF))
                            a = F(w * F(pcm[i]))
                            c = F(F(F(1) - w) * F(int(tmp[i]) - delta))
                            self.count["blend_wrap"] += _wraps(math.floor((.5 + float(a)) + float(c)))
                            pcm[i] = _short(math.floor((.5 + float(a)) + float(c)))
                    self._t(IMPL, HALF, CI_PCM_PRE)  # :231
                    if not stub:
                        self.lpcnet.synthesize(self.features, HALF, preload=pcm[:HALF])
                else:
                    if self.delay > 0:
                        self._plc_restore(self.delay - 1)  # :233
                    self._t(FEC_REWIND, self.delay)  # :234, :168-173
                    self.fec_read_pos = max(self.fec_read_pos - self.delay, self.fec_keep_pos)
                    self._t(RESET_SIGNAL)  # :236
                    if not stub:
                        self.lpcnet.reset_signal()
                self._t(PCM_MOVE, CM_TAIL_HALF)  # :242-243
                self._moved(TRAINING_OFFSET)
                self.pcm[:TRAINING_OFFSET] = pcm[HALF:]
                self.pcm_fill = TRAINING_OFFSET
            else:
                self._t(PCM_MOVE, CM_APPEND, self.pcm_fill)  # :245-246
                self._moved(FRAME_SIZE)
                self.pcm[self.pcm_fill:self.pcm_fill + FRAME_SIZE] = pcm
                self.pcm_fill += FRAME_SIZE
        enc_features = self._analysis(pcm)  # :251-254
        if not self.blend:
            if not stub:
                plc_features[2 * NB_BANDS:2 * NB_BANDS + NB_FEATURES] = enc_features  # :256-257
                plc_features[-1] = 1
            self._pred(CP_FULL, plc_features)  # :258
            self._t(FEC_DISCARD)  # :260-262
            if self.fec_skip:
                self.fec_skip -= 1
            elif self.fec_read_pos < self.fec_fill_pos:
                self.fec_read_pos += 1
            self._keep_pos()
        if self.skip_analysis:
            if self.enable_blending:
                self._deferred(CD_ANALYSED, enc_features)  # :267
            self.skip_analysis -= 1
        else:
            self._t(PCM_MOVE, CM_NEWEST)  # :271
            self._moved(FRAME_SIZE)
            self.pcm[self.buf:] = pcm
            self._deferred(CD_ANALYSED, enc_features)  # :275 (PLC_SKIP_UPDATES)
            self._shift()  # :280
        self.loss_count = 0
        if self.remove_dc:  # :283-287
            self._t(DC_RESTORE)
            for i in range(FRAME_SIZE):
                self.count["dc_add_wrap"] += _wraps(int(pcm[i]) + int(lp[i]))
                pcm[i] = _short(int(pcm[i]) + int(lp[i]))
        self.blend = 0
        return pcm

    # -- lpcnet_plc_conceal_causal (:293-337) -----------------------------------------
    def conceal(self) -> np.ndarray:
        stub = self.stub
        pcm = np.zeros(FRAME_SIZE, np.int16)
        for j in range(self.feature_buffer_fill):  # :296, lpcnet.c:134-144
            self._t(FLUSH, j)
        self.feature_buffer_fill = 0
        if not stub:
            self.lpcnet.frame_flush()
        while self.pcm_fill > 0:  # :300-312
            n = min(self.pcm_fill, FRAME_SIZE)
            output = self.pcm[:n].copy()
            self._plc_push()
            self._get_fec_or_pred()
            self._t(IMPL, n, CI_BUF)
            if not stub:
                self.lpcnet.synthesize(self.features, n, preload=output)
            self._shift()
            self.pcm_fill -= n
            self.skip_analysis += 1
        self._plc_push()  # :313-314
        self._t(TAIL, HALF)  # :315
        if not stub:
            pcm[:HALF] = self.lpcnet.synthesize_tail(np.zeros(HALF, np.int16), 0)
        if self._get_fec_or_pred():  # :316-317
            self.loss_count = 0
        else:
            self.loss_count += 1
        self._t(ATTENUATE, self.loss_count)  # :318-319
        f0 = self.features[0]
        if self.loss_count >= 10:
            v = F(F(f0 + ATT_TABLE[9]) - F(2 * (self.loss_count - 9)))
        else:
            v = F(f0 + ATT_TABLE[self.loss_count])
        self.count["loss_ge_10"] += self.loss_count >= 10
        self.count["clamp"] += bool(-10 > v)
        self.features[0] = F(-10) if -10 > v else v
        self._t(IMPL, TRAINING_OFFSET, CI_PCM_OUT)  # :320
        if not stub:
            pcm[HALF:] = self.lpcnet.synthesize(self.features, TRAINING_OFFSET)
        self._analysis(pcm)  # :322-328
        self.blend = 1
        if self.remove_dc:  # :330-335
            self._t(DC_CONCEAL)
            add = int(math.floor(.5 + self.dc_mem))
            self.count["l_negative"] += add < 0
            for i in range(FRAME_SIZE):
                self.syn_dc += DC_CONST * (float(pcm[i]) - self.syn_dc)
                self.count["dc_add_wrap"] += _wraps(int(pcm[i]) + add)
                pcm[i] = _short(int(pcm[i]) + add)
        return pcm

    def tick(self, pcm, lost: bool) -> np.ndarray:
        """lpcnet_plc_update (pcm in/out) or lpcnet_plc_conceal (:495-503)."""
        return self.conceal() if lost else self.update(pcm)

    def take_trace(self) -> list:
        t, self.trace = self.trace, []
        return t


# -- the fixture's scripts ----------------------------------------------------------

NTICKS = 28
SCRIPTS = [
    "G" * 28,                             # steady state
    "GGGGL" + "G" * 23,                   # one loss, the whole skip_analysis countdown
    "GGLLGL" + "G" * 22,                  # a loss with skip_analysis > 0 and pcm_fill == 80: the loop runs once
    "GGGLGLLGGL" + "GGGGGG" + "LG" * 6,   # a loss with pcm_fill == 240: the loop runs 160 then 80; then every other tick
    "LLGG" + "L" * 12 + "G" * 12,         # a loss before any frame; loss_count >= 10
    "GGLLGLGGLLLLGG" + "GGG" + "LG" * 5 + "L",  # script 2's start with FEC; ends on a lost tick
]
# FEC events before each tick of script 5 (index): n > 0 adds, -1 a NULL add,
# -2 a clear.  Adds before the losses, a NULL add, a stretch that runs the
# queue dry (ticks 8-11 against what is left) and a clear.
FEC_EVENTS = {0: 3, 1: -1, 2: 2, 5: 1, 7: 2, 10: -2, 11: 1, 20: 4}
SIGNALS = ["chirp_up", "stair_dn4", "two45_90", "noise_pulse", "p33", "fullnoise"]
# (name, options, FEATURES_DELAY) of the fixture's runs
RUNS = [("causal", CAUSAL, 2), ("codec", CODEC, 2), ("causal_dc", CAUSAL | DC_FILTER, 2), ("causal_d0", CAUSAL, 0),
        ("causal_plc", CAUSAL, 2)]  # the last one on the predictor's default shape, the others on the small one
assert all(len(s) == NTICKS for s in SCRIPTS)


def lost_matrix() -> np.ndarray:
    """[6, 28] uint8, 1 = lost."""
    return np.array([[c == "L" for c in s] for s in SCRIPTS], np.uint8)


def fec_events(stream: int) -> np.ndarray:
    """[28] int32 event codes of one script's stream (only script 5 has any)."""
    ev = np.zeros(NTICKS, np.int32)
    if stream == len(SCRIPTS) - 1:
        for t, v in FEC_EVENTS.items():
            ev[t] = v
    return ev


def fec_row(k: int) -> np.ndarray:
    """The k-th FEC frame a script adds: features [20]."""
    import lpcnet_amd as L
    return L.synthetic_features(3000 + k, 1)[0, :NB_FEATURES].copy()


def received_pcm() -> np.ndarray:
    """[6, 28, 160] int16: the scripts' received frames (a lost tick's row is unused)."""
    import feat_signals as FS
    out = np.zeros((len(SIGNALS), NTICKS, FRAME_SIZE), np.int16)
    for s, name in enumerate(SIGNALS):
        p = FS.pcm_of(name)
        assert p.dtype == np.int16
        out[s] = p[np.arange(NTICKS) % len(p)]
    return out


def run_script(ref: ConcealRef, stream: int, pcm: np.ndarray, on_received=None):
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


def model_blob(run: str) -> bytes:
    import lpcnet_amd as L
    big = run == "causal_plc"
    return L.synthetic_model(1, L.VARIANT_INT8, codebooks=False, plc=big, plc_small=not big)


def check_received(ref: ConcealRef, pcm: np.ndarray) -> None:
    """A received frame, DC-removed as the update will see it, must be inside
    Burg's contract (the reference asserts otherwise): fail loudly."""
    import burg_ref
    p = np.array(pcm, np.int16)
    if ref.remove_dc:
        dc_mem = ref.dc_mem + ref.syn_dc
        for i in range(FRAME_SIZE):
            l = _short(math.floor(.5 + dc_mem))
            dc_mem += DC_CONST * (float(p[i]) - dc_mem)
            p[i] = _short(int(p[i]) - l)
    for h in (p[:HALF], p[HALF:]):
        if not h.any():
            raise ValueError("an all-zero half-frame reaches burg_cepstral_analysis")
    ceps = burg_ref.burg_frame(p)[0]
    if not np.isfinite(ceps).all():
        raise ValueError("burg_cepstral_analysis is not finite on a received frame")


def compute_run(run: str, options: int, delay: int, streams=None, check: bool = True) -> dict:
    """The arrays of one run of the fixture (keys without the run's prefix)."""
    blob = model_blob(run)
    pcm_in = received_pcm()
    streams = range(len(SCRIPTS)) if streams is None else streams
    out = {k: [] for k in ("pcm", "ctrl", "features", "buf", "dc", "gru_a", "gru_b", "frame_count", "plc", "enc")}
    for s in streams:
        ref = ConcealRef(blob, options, delay)
        out["pcm"].append(run_script(ref, s, pcm_in[s], check_received if check else None))
        c = ref.ctrl()
        out["ctrl"].append(np.array([c[k] for k in CTRL], np.int32))
        out["features"].append(ref.features.copy())
        out["buf"].append(ref.pcm.copy())
        out["dc"].append(np.array([ref.dc_mem, ref.syn_dc], np.float64))
        a, b = ref.lpcnet.state()
        out["gru_a"].append(a)
        out["gru_b"].append(b)
        out["frame_count"].append(ref.lpcnet.frame_count())
        out["plc"].append(np.frombuffer(ref.net.save(), F).copy())
        out["enc"].append(np.frombuffer(ref.enc.state_bytes(), np.uint8).copy())
    return {k: np.stack(v) if k != "frame_count" else np.array(v, np.int32) for k, v in out.items()}


COMPACT_TICKS = 6
COMPACT_LOST = [0, 0, 1, 1, 1, 1]
COMPACT_ADD_AT = 4  # the add before this tick finds the queue full with fec_keep_pos > 0


def compaction_adds(t: int) -> list:
    """The FEC frames added before tick t of the compaction scenario: 100
    before the first tick, one more before tick COMPACT_ADD_AT (lpcnet_plc.c:121-124)."""
    if t == 0:
        return [fec_row(k % 11) for k in range(PLC_MAX_FEC)]
    return [fec_row(3)] if t == COMPACT_ADD_AT else []


def compute_compaction() -> dict:
    """One codec-mode stream on signal 0: the queue filled to the brim, two
    received ticks, then losses that read from it; the add in their middle
    compacts it.  pcm [6, 160], ctrl [9], features [20]."""
    ref = ConcealRef(model_blob("codec"), CODEC, 2)
    pcm_in = received_pcm()[0]
    out = []
    for t in range(COMPACT_TICKS):
        if t == COMPACT_ADD_AT:
            assert ref.fec_fill_pos == PLC_MAX_FEC and ref.fec_keep_pos > 0
        for row in compaction_adds(t):
            assert ref.fec_add(row)
        out.append(ref.tick(pcm_in[t], bool(COMPACT_LOST[t])))
    c = ref.ctrl()
    return {"pcm": np.stack(out), "ctrl": np.array([c[k] for k in CTRL], np.int32), "features": ref.features.copy()}


_fix = None


def fixture() -> dict:
    """The committed fixture, read-only.  pcm_in [6, 28, 160]; compact_pcm,
    compact_ctrl, compact_features (compute_compaction); per run r of
    RUNS: r_pcm [6, 28, 160], r_ctrl [6, 9], r_features [6, 20], r_buf
    [6, PLC_BUF_SIZE + 160], r_dc [6, 2] float64, r_gru_a [6, 384], r_gru_b
    [6, 16], r_frame_count [6], r_plc [6, n1 + n2] float32 and r_enc
    [6, state bytes] uint8."""
    global _fix
    if _fix is None:
        with np.load(GOLDEN) as g:
            _fix = {k: g[k] for k in g.files}
        for v in _fix.values():
            v.setflags(write=False)
    return _fix
