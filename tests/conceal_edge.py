"""The concealment machine's edge cases: every FEATURES_DELAY, PCM that makes
the DC filter's short stores wrap and its integer conversions see negative
fractions, and FEC rows that are not ordinary features.  The cases, the
generators of their inputs, the computation of their answers through
tests/conceal_ref.py and tests/conceal_nc_ref.py, and what the CPU and GPU
tests share: the loader of the fixture tests/golden/conceal_edge.npz
(tests/golden/make_conceal_edge_golden.py writes it), the digest of a large
state and the comparison of a final state.

Three run sets, each run a group of streams from lpcnet_plc_reset over 28
ticks (a case = one stream: a script, a signal, its FEC rows):
  D  the delays: the six scripts of conceal_ref.SCRIPTS on
     conceal_ref.received_pcm() with script 5's FEC events, at the (options,
     FEATURES_DELAY) pairs of RUNS_D;
  E  edge PCM: the five signals of EDGE_SIGNALS, each on script 3 and on the
     long burst (LONG_BURST), with the DC filter in the runs of RUNS_E, the
     last of them non-causal;
  T  rounding ties: three of set D's signals with their first two samples
     replaced so that dc_mem is 4.5, 10.5 and 16.5 exactly when the second
     sample's floor(.5 + dc_mem) is taken (TIE_CASES), causal with the DC filter
     at FEATURES_DELAY 2;
  F  edge FEC rows: script 5 in the codec mode at FEATURES_DELAY 2 on signal
     5, the queued rows taken from tests/cond_frames.py's edge frames
     (F_CASES).
The tests read inputs and answers from the fixture and never call a
generator.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import hashlib
import os

import numpy as np

import conceal_nc_ref as NR
import conceal_ref as CR
from conceal_ref import CAUSAL, CODEC, DC_FILTER, FRAME_SIZE, NB_FEATURES, NONCAUSAL, NTICKS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conceal_edge.npz")
SEED = 20261022
NAN = 0x7FC00000

# -- scripts --------------------------------------------------------------------------
LONG_BURST = "GGG" + "L" * 20 + "G" * 5  # loss_count >= 10 for eleven ticks; the attenuation walks features[0] to the clamp
SCRIPTS = CR.SCRIPTS + [LONG_BURST]
FEC_SCRIPT, EVERY_OTHER, BURST = 5, 3, 6
assert all(len(s) == NTICKS for s in SCRIPTS)


def lost_matrix() -> np.ndarray:
    """[7, 28] uint8, 1 = lost."""
    return np.array([[c == "L" for c in s] for s in SCRIPTS], np.uint8)


def fec_events(script: int) -> np.ndarray:
    return CR.fec_events(script)  # only script 5 has any


NROWS = sum(v for v in CR.FEC_EVENTS.values() if v > 0)  # the rows script 5 adds

# -- edge signals ---------------------------------------------------------------------
EDGE_SIGNALS = [
    "dc_hi_tone",  # 30000 + 2500 sin: dc_mem near +30000 and, with syn_dc, beyond int16; pcm + add wraps on a lost tick
    "dc_lo_tone",  # -30500 + 2000 sin: l, add and delta negative, (int)syn_dc above floor(syn_dc)
    "square_fs",   # +-full scale, period 80: every product of the blend at the top of int16
    "fullnoise",   # tests/feat_signals.py's: every int16 value
    "dc_step",     # DC +20000 until frame 10, -20000 after: pcm - l wraps, dc_mem crosses zero while syn_dc is live
]
STEP_FRAME = 10


def rng_of(name: str) -> np.random.RandomState:
    return np.random.RandomState(SEED + EDGE_SIGNALS.index(name))


def make_signal(name: str) -> np.ndarray:
    """[28, 160] int16."""
    n = NTICKS * FRAME_SIZE
    i = np.arange(n)
    rng = rng_of(name)
    if name == "dc_hi_tone":
        y = 30000 + 2500 * np.sin(2 * np.pi * i / 57.3) + rng.randint(-30, 31, n)
    elif name == "dc_lo_tone":
        y = -30500 + 2000 * np.sin(2 * np.pi * i / 91.7) + rng.randint(-30, 31, n)
    elif name == "square_fs":
        y = np.where(i % 80 < 40, 32767, -32768)
    elif name == "fullnoise":
        return NR.signal_pcm("fullnoise").copy()
    elif name == "dc_step":
        y = np.where(i < STEP_FRAME * FRAME_SIZE, 20000, -20000) + 3000 * np.sin(2 * np.pi * i / 71.9) + rng.randint(-30, 31, n)
    else:
        raise KeyError(name)
    return np.clip(np.rint(y), -32768, 32767).astype(np.int16).reshape(NTICKS, FRAME_SIZE)


# -- runs -----------------------------------------------------------------------------
# (name, options, FEATURES_DELAY)
RUNS_D = [("d_causal_1", CAUSAL, 1), ("d_causal_3", CAUSAL, 3), ("d_causal_4", CAUSAL, 4),
          ("d_codec_1", CODEC, 1), ("d_codec_4", CODEC, 4),
          ("d_causal_dc_0", CAUSAL | DC_FILTER, 0), ("d_causal_dc_1", CAUSAL | DC_FILTER, 1), ("d_causal_dc_4", CAUSAL | DC_FILTER, 4),
          ("d_codec_dc_2", CODEC | DC_FILTER, 2), ("d_codec_dc_3", CODEC | DC_FILTER, 3)]
RUNS_E = [("e_causal_dc_2", CAUSAL | DC_FILTER, 2), ("e_causal_dc_4", CAUSAL | DC_FILTER, 4), ("e_codec_dc_0", CODEC | DC_FILTER, 0),
          ("e_noncausal_dc_0", NONCAUSAL | DC_FILTER, 0)]
RUNS_T = [("t_causal_dc_2", CAUSAL | DC_FILTER, 2)]
RUNS_F = [("f_codec_2", CODEC, 2)]
RUNS = RUNS_D + RUNS_E + RUNS_T + RUNS_F
RUN = {r[0]: r for r in RUNS}
E_CASES = [(sig, script) for sig in range(len(EDGE_SIGNALS)) for script in (EVERY_OTHER, BURST)]  # stream 2 sig + (script == 6)
# stream -> the 13 rows script 5 queues, as (sequence of tests/cond_frames.py, frame) or (sequence, frame, i, j): that
# frame with features i and j exchanged; a non-finite row poisons what follows it in its stream, so each kind has a
# stream of its own.  Row k (from 0) reaches the attenuation and the tick's own synthesis at ticks 2 and 5 (k = 4), 8 (6),
# 9 (7), 11 and 19 (8) and 21 .. 27 (9); rows 1 .. 9 are all fetched
F_CASES = [
    ("extremes", [("loud", 0), ("lpc_wide", 0), ("lpc_wide", 1), ("corr_edges", 2), ("corr_edges", 3), ("alt_sign", 1),
                  ("loud", 1), ("lpc_wide", 2), ("lpc_wide", 3), ("lpc_wide", 4), ("lpc_wide", 5), ("scale_lo", 11), ("lpc_wide", 6)]),
    ("zeros_subnormals", [("neg_zeros", 0), ("subnormal", 0), ("tiny", 0), ("zeros", 0), ("scale_lo", 0), ("neg_zeros", 1),
                          ("subnormal", 1), ("scale_lo", 3), ("tiny", 1), ("neg_zeros", 2), ("subnormal", 2), ("scale_lo", 5),
                          ("zeros", 1)]),
    ("pitch_clamps", [("pitch_edges2", f) for f in range(5, 12)] + [("pitch_edges3", f) for f in range(6)]),
    # NaN in band 3 of row 9, the row the last four lost ticks synthesise from: the final state holds it
    ("nan_row", [("const", f) for f in range(9)] + [("nan_band", 5)] + [("const", f) for f in range(9, 12)]),
    # NaN in features[0] of row 4, which ticks 2 and 5 attenuate: -10.f > v ? -10.f : v keeps it (MAX16), fmaxf would
    # return -10; the received ticks after them reset the signal and the later rows are finite
    ("nan_c0", [("const", f) for f in range(4)] + [("nan_band", 5, 0, 3)] + [("const", f) for f in range(4, 12)]),
    # c0 = +inf in row 6 (tick 8 attenuates it), -inf in row 9 (the last lost ticks: the clamp gives -10)
    ("inf_row", [("const", f) for f in range(6)] + [("inf_c0", 4), ("const", 6), ("const", 7), ("inf_c0", 8)]
     + [("const", f) for f in range(8, 11)]),
    # finite in, not finite inside: band 7 = 3e38 in row 4, features[18] = +-1e10 in rows 6 and 7
    ("huge_finite", [("const", f) for f in range(4)] + [("max_float", 5), ("const", 4), ("pitch_huge", 0), ("pitch_huge", 1)]
     + [("const", f) for f in range(5, 10)]),
]
F_NONFINITE = ("nan_row", "nan_c0", "inf_row", "huge_finite")  # the reference's float state may hold NaN
assert all(len(rows) == NROWS for _, rows in F_CASES)
F_SIGNAL = 5  # script 5's own signal of conceal_ref.SIGNALS


def f_rows() -> np.ndarray:
    """[7, 13, 20] float32: the rows the streams of set F queue."""
    import cond_frames as CF

    def row(seq, f, i=0, j=0):
        r = CF.features_of(seq)[f, :NB_FEATURES].astype(np.float32)
        r[[i, j]] = r[[j, i]]
        return r
    return np.stack([np.stack([row(*spec) for spec in rows]) for _, rows in F_CASES])


# (signal of conceal_ref.SIGNALS, script, first sample): .003 * 1500 = 4.5, * 3500 = 10.5 and * 5500 = 16.5 exactly in
# double (dc_mem is 0 after a reset), the only ties a signal can stage: floor(.5 + dc_mem) gives 5, 11, 17 for the second
# sample's l where rint(dc_mem) gives 4, 10, 16.  The second sample is 3: the DC-removed one lies where mu-law is fine.
TIE_CASES = [(0, 1, 1500), (1, EVERY_OTHER, 3500), (3, BURST, 5500)]


def tie_pcm() -> np.ndarray:
    """[3, 28, 160] int16."""
    out = np.stack([CR.received_pcm()[sig] for sig, _, _ in TIE_CASES])
    for k, (_, _, first) in enumerate(TIE_CASES):
        out[k, 0, 0], out[k, 0, 1] = first, 3
    return out


def nstreams(run: str) -> int:
    return {"d": len(CR.SCRIPTS), "e": len(E_CASES), "t": len(TIE_CASES), "f": len(F_CASES)}[run[0]]


def script_of(run: str, s: int) -> int:
    return s if run.startswith("d_") else E_CASES[s][1] if run.startswith("e_") else TIE_CASES[s][1] if run.startswith("t_") else FEC_SCRIPT


def model_blob() -> bytes:
    return CR.model_blob("causal")  # the small predictor shape, as in every run of the other fixtures but causal_plc


# -- the answers ----------------------------------------------------------------------
BIG = ("gru_a", "plc", "enc")  # stored as digests in sets D and E, in full in set F
NC_KEYS = ("queued_update", "queued_samples", "dcbuf")


def canon(a) -> bytes:
    """The bytes of a float32 state with every NaN as 0x7FC00000 (x86 makes 0xFFC00000, the device 0x7FC00000)."""
    if isinstance(a, (bytes, bytearray)):
        a = np.frombuffer(a, np.uint32)
    w = np.ascontiguousarray(a).view(np.uint32).copy()
    w[np.isnan(w.view(np.float32))] = NAN
    return w.tobytes()


def digest(a, floats: bool = True) -> np.ndarray:
    """[32] uint8: SHA-256 of a state (float32 states canonical in their NaNs, the analysis state as it is: it holds ints)."""
    data = canon(a) if floats else bytes(a)
    return np.frombuffer(hashlib.sha256(data).digest(), np.uint8)


def play(ref, script: int, pcm: np.ndarray, rows, on_received) -> np.ndarray:
    """Script `script` on ``ref`` from reset, the FEC events before each tick
    drawing from ``rows``: the PCM of every tick [28, 160]."""
    lost, ev = lost_matrix()[script], fec_events(script)
    out = np.zeros((NTICKS, FRAME_SIZE), np.int16)
    k = 0
    for t in range(NTICKS):
        if ev[t] == -2:
            ref.fec_clear()
        elif ev[t] == -1:
            ref.fec_add(None)
        for _ in range(max(0, int(ev[t]))):
            assert ref.fec_add(rows[k])
            k += 1
        if not lost[t]:
            on_received(ref, pcm[t])  # Burg's contract: a condition on the inputs, never waived
        out[t] = ref.tick(pcm[t], bool(lost[t]))
    return out


def inputs(run: str) -> tuple:
    """(pcm_in [S, 28, 160], rows [S] of [13, 20] or None) of a run, from the generators."""
    if run.startswith("d_"):
        fec = np.stack([CR.fec_row(k) for k in range(NROWS)])
        return CR.received_pcm(), [fec if s == FEC_SCRIPT else None for s in range(len(CR.SCRIPTS))]
    if run.startswith("e_"):
        sig = [make_signal(n) for n in EDGE_SIGNALS]
        return np.stack([sig[g] for g, _ in E_CASES]), [None] * len(E_CASES)
    if run.startswith("t_"):
        return tie_pcm(), [None] * len(TIE_CASES)
    return np.stack([CR.received_pcm()[F_SIGNAL]] * len(F_CASES)), list(f_rows())


def compute_run(run: str, streams=None) -> tuple:
    """(the arrays of one run, keys without the run's prefix; the counters of
    its streams, a list of conceal_ref.COUNTERS dicts)."""
    _, options, delay = RUN[run]
    nc = options & 3 == NONCAUSAL
    blob = model_blob()
    pcm_in, rows = inputs(run)
    full = run.startswith("f_")
    keys = ("pcm", "ctrl", "features", "buf", "dc", "gru_b", "frame_count") + (BIG if full else ("digests",)) + (NC_KEYS if nc else ())
    out = {k: [] for k in keys}
    counts = []
    for s in (range(len(pcm_in)) if streams is None else streams):
        ref = NR.ConcealNcRef(blob, options) if nc else CR.ConcealRef(blob, options, delay)
        out["pcm"].append(play(ref, script_of(run, s), pcm_in[s], rows[s], NR.check_received if nc else CR.check_received))
        c = ref.ctrl()
        out["ctrl"].append(np.array([c[k] for k in CR.CTRL], np.int32))
        out["features"].append(ref.features.copy())
        out["buf"].append(ref.pcm.copy())
        out["dc"].append(np.array([ref.dc_mem, ref.syn_dc], np.float64))
        a, b = ref.lpcnet.state()
        out["gru_b"].append(b)
        out["frame_count"].append(np.int32(ref.lpcnet.frame_count()))
        big = {"gru_a": a, "plc": np.frombuffer(ref.net.save(), np.float32).copy(),
               "enc": np.frombuffer(ref.enc.state_bytes(), np.uint8).copy()}
        if full:
            for k in BIG:
                out[k].append(big[k])
        else:
            out["digests"].append(np.stack([digest(big[k], k != "enc") for k in BIG]))
        if nc:
            out["queued_update"].append(np.int32(ref.queued_update))
            out["queued_samples"].append(ref.queued_samples.copy())
            out["dcbuf"].append(ref.dc_buf.copy())
        counts.append(dict(ref.count))
    return {k: np.stack(v) for k, v in out.items()}, counts


def compute_inputs() -> dict:
    return {"lost": lost_matrix(), "fec_events": np.stack([fec_events(s) for s in range(len(SCRIPTS))]),
            "edge_pcm": np.stack([make_signal(n) for n in EDGE_SIGNALS]), "tie_pcm": tie_pcm(), "f_rows": f_rows()}


# -- the fixture ----------------------------------------------------------------------
SETS = {"d": RUNS_D, "e": RUNS_E}


def pack(arrays: dict) -> dict:
    """The file's layout: the PCM of the runs of set D as one array d_pcm
    [S, 28, runs, 160], likewise e_pcm.  A received frame comes back the same
    in most runs, and side by side the compressor sees it; every sample of
    every tick is there."""
    out = dict(arrays)
    for name, runs in SETS.items():
        out[f"{name}_pcm"] = np.stack([out.pop(f"{r}_pcm") for r, _, _ in runs], axis=2)
    return out


def unpack(arrays: dict) -> dict:
    out = dict(arrays)
    for name, runs in SETS.items():
        both = out.pop(f"{name}_pcm")
        for i, (r, _, _) in enumerate(runs):
            out[f"{r}_pcm"] = np.ascontiguousarray(both[:, :, i])
    return out


_fix = None


def fixture() -> dict:
    """The committed fixture, read-only, unpacked.  lost, fec_events [7, 28]; edge_pcm
    [5, 28, 160] (EDGE_SIGNALS); tie_pcm [3, 28, 160] (TIE_CASES); f_rows [7, 13, 20]; per run r of RUNS with S
    streams: r_pcm [S, 28, 160], r_ctrl [S, 9], r_features [S, 20], r_buf
    [S, PLC_BUF_SIZE + 160], r_dc [S, 2] float64, r_gru_b [S, 16],
    r_frame_count [S]; in sets D and E r_digests [S, 3, 32] uint8 (digest() of
    the GRU_A state, the predictor's state and the analysis state; set T
    likewise), in set F
    r_gru_a [S, 384], r_plc [S, n1 + n2] and r_enc [S, state bytes] themselves;
    in the non-causal run also r_queued_update [S], r_queued_samples
    [S, 160] and r_dcbuf [S, 80]."""
    global _fix
    if _fix is None:
        with np.load(GOLDEN) as g:
            _fix = unpack({k: g[k] for k in g.files})
        for v in _fix.values():
            v.setflags(write=False)
    return _fix


def run_inputs(run: str) -> dict:
    """What a driver of a run reads, by stream: lost, fec_events, pcm_in, rows
    (from the committed fixtures alone) and `run`_pcm, the answer."""
    fx = fixture()
    S = nstreams(run)
    sc = [script_of(run, s) for s in range(S)]
    if run.startswith("d_"):
        pcm_in = CR.fixture()["pcm_in"]
        rows = np.stack([CR.fec_row(k) for k in range(NROWS)])[None].repeat(S, 0)
    elif run.startswith("e_"):
        pcm_in = np.stack([fx["edge_pcm"][g] for g, _ in E_CASES])
        rows = np.zeros((S, NROWS, NB_FEATURES), np.float32)
    elif run.startswith("t_"):
        pcm_in = fx["tie_pcm"]
        rows = np.zeros((S, NROWS, NB_FEATURES), np.float32)
    else:
        pcm_in = np.stack([CR.fixture()["pcm_in"][F_SIGNAL]] * S)
        rows = fx["f_rows"]
    return {"lost": fx["lost"][sc], "fec_events": fx["fec_events"][sc], "pcm_in": pcm_in, f"{run}_pcm_in": pcm_in, "rows": rows,
            f"{run}_pcm": fx[f"{run}_pcm"]}


def same_floats(dev, ref, nonfinite: bool) -> bool:
    """tests/tile_cases.py's rule: where the reference is NaN the device must
    hold a quiet NaN, everywhere else the bits are equal; a reference NaN in
    a stream not listed as non-finite never compares equal."""
    import tile_cases as TC
    return TC.same(dev, ref, nonfinite)


def check_final_state(b, run: str, s: int, c: int) -> None:
    """Stream s of the batch against case c of a run: every field of
    tests/test_gpu_conceal.py's check_final_state (and of the non-causal one
    in that mode)."""
    fx = fixture()
    _, options, _ = RUN[run]
    nonfinite = run.startswith("f_") and F_CASES[c][0] in F_NONFINITE
    st = b.conceal_state(s)
    assert [st[k] for k in CR.CTRL] == fx[f"{run}_ctrl"][c].tolist(), (run, c, "control fields")
    assert same_floats(st["features"], fx[f"{run}_features"][c], nonfinite), (run, c, "st->features")
    assert np.array_equal(st["pcm"], fx[f"{run}_buf"][c]), (run, c, "st->pcm")
    assert np.array([st["dc_mem"], st["syn_dc"]]).tobytes() == fx[f"{run}_dc"][c].tobytes(), (run, c, "dc_mem / syn_dc")
    g = b.get_state(s)
    assert same_floats(g["gru_b_state"], fx[f"{run}_gru_b"][c], nonfinite), (run, c, "GRU_B state")
    assert g["frame_count"] == fx[f"{run}_frame_count"][c], (run, c, "frame_count")
    big = {"gru_a": g["gru_a_state"], "plc": b.plc_save_state(s), "enc": b.features_save_state(s)}
    if run.startswith("f_"):
        assert same_floats(big["gru_a"], fx[f"{run}_gru_a"][c], nonfinite), (run, c, "GRU_A state")
        assert same_floats(big["plc"], fx[f"{run}_plc"][c], nonfinite), (run, c, "predictor state")
        assert big["enc"] == fx[f"{run}_enc"][c].tobytes(), (run, c, "analysis state")
    else:
        for i, k in enumerate(BIG):
            assert np.array_equal(digest(big[k], k != "enc"), fx[f"{run}_digests"][c, i]), (run, c, k + " state (digest)")
    if options & 3 == NONCAUSAL:
        nc = b.conceal_state_noncausal(s)
        assert nc["queued_update"] == fx[f"{run}_queued_update"][c], (run, c, "queued_update")
        assert np.array_equal(nc["queued_samples"], fx[f"{run}_queued_samples"][c]), (run, c, "queued_samples")
        assert np.array_equal(nc["dc_buf"], fx[f"{run}_dcbuf"][c]), (run, c, "dc_buf")
