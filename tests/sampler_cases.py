"""The edge cases of the sample kernels' sampler role -- the GRU_B update, the
dual-FC tree walk (nnet.c:163-214), the kiss99 thresholds and the signal tail
of lpcnet.c:235-271 (pred, u-law, teacher forcing, de-emphasis, clamp,
rounding) -- shared by tests/golden/make_sampler_golden.py (which writes
tests/golden/sampler_edge.npz from them through the CPU oracle), the CPU test
tests/test_sampler_cases_ref.py and the GPU test tests/test_gpu_sampler_edge.py.

Three classes of case, each a 14-frame run on one stream (SCHEDULE):

* TAILS: a hand-written tail state (last_sig, deemph_mem, last_exc, the four
  kiss99 words, one with a NaN GRU_B state) put into a running stream after
  frame 3, on the plain int8, fp32 and saturating int8 models;
* EDITED: models whose dual-FC or GRU_B / GRU_A-conditioning records are
  edited so that the walk meets threshold ties, NaN / inf logits, both tanh
  forms, saturated states and out-of-range int8 seeds;
* NONFINITE: the non-finite conditioning sequences of tests/cond_frames.py
  (plus loud and lpc_wide) through synthesis, on the plain models.

TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import functools
import hashlib
import os

import numpy as np

import cond_frames as CF
import lpcnet_amd as L
import oracle_lib as O
from cond_frames import STATE, _floats, _put_floats  # noqa: F401  (STATE is re-exported)
from test_ingest import find, join, records

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_edge.npz")
SEED = 20261101
F32 = np.float32
NFRAMES, FRAME, NF = 14, L.FRAME_SIZE, 20
NB, NA, NLEVELS = 16, 384, 256
NAN = 0x7FC00000
VARIANTS = {"int8": L.VARIANT_INT8, "fp32": L.VARIANT_FP32}
# the plain models the tail states run on: the two above and the saturating int8 model ("sat": maddubs pair sums
# that reach the int16 limits), which only the lockstep sample kernel runs
PLAIN = {"int8": (L.VARIANT_INT8, False), "fp32": (L.VARIANT_FP32, False), "sat": (L.VARIANT_INT8, True)}

# the run: frame -> (entry point, samples, teacher-forced samples); frames 10..13 are one device-resident
# lpcnet_batch_synthesize_frames call on the GPU (multi-frame launches keep the sampler state in registers)
TAIL_AFTER = 3          # the tail state is written after this frame
DEVICE_FRAMES = (10, 14)
SCHEDULE = {f: (FRAME, 0) for f in range(NFRAMES)}
SCHEDULE[5] = (FRAME, 77)   # teacher alternates 32767 / -32768
SCHEDULE[7] = (FRAME, 160)  # teacher 32767 sin(0.3 t + phase)
SCHEDULE[8] = (81, 0)
SCHEDULE[9] = (1, 0)


def logit_table() -> np.ndarray:
    """lpcnet.c:188-191 in float32: prob in float, the quotient in float, log in double."""
    i = np.arange(256, dtype=np.float32)
    prob = F32(.025) + F32(.95) * i / F32(255)
    q = (F32(1) - prob) / prob
    return (-np.log(q.astype(np.float64))).astype(np.float32)


LT = logit_table()

# -- edited models ---------------------------------------------------------------------------

EDITED = ["fc_tie", "fc_ramp", "fc_mid", "fc_factor", "fc_hi", "fc_lo", "gb_sat", "gb_in_over", "gb_both_over", "gb_nonfinite",
          "ga_hbias", "ga_zrbias"]
FACTORS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e38, -1e38, 1e-42], np.float32)


def _edit_fc(recs, name: str) -> None:
    rw, rb, rf = (find(recs, n) for n in ("dual_fc_weights", "dual_fc_bias", "dual_fc_factor"))
    w = _floats(rw).reshape(NLEVELS, 2, NB)
    b = _floats(rb).reshape(2, NLEVELS)
    f = _floats(rf).reshape(2, NLEVELS)
    if name in ("fc_tie", "fc_hi", "fc_lo"):
        w[:] = 0
        b[:] = F32(1e3)  # tanh(1e3) = 1 exactly: a logit is factor[0] + factor[1]
        if name == "fc_tie":
            f[0] = LT[(37 * np.arange(NLEVELS)) & 255]
            f[1] = 0
        else:
            f[:] = F32(8 if name == "fc_hi" else -8)
    elif name in ("fc_ramp", "fc_mid"):
        s = (10.0 ** (np.arange(NLEVELS) % (24 if name == "fc_ramp" else 15))).astype(np.float32)
        w *= s[:, None, None]
        b *= s[None, :]
    elif name == "fc_factor":
        flat = f.reshape(-1)
        idx = np.arange(2, flat.size, 5)
        flat[idx] = FACTORS[np.arange(idx.size) % FACTORS.size]
    _put_floats(rw, w)
    _put_floats(rb, b)
    _put_floats(rf, f)


def _edit_gb(recs, name: str) -> None:
    for rec in ("gru_b_bias", "gru_b_subias"):
        r = find(recs, rec)
        v = _floats(r)
        assert v.size == 6 * NB
        if name == "gb_sat":
            v[0:16] = -40
            v[32:48] = 40 * (-1.0) ** np.arange(16)
        elif name == "gb_in_over":
            v[0:16:3] = 1e6
            v[32:48:4] = 1e6
            v[16:32:5] = -1e6
        elif name == "gb_both_over":
            v[0:16:3] = 1e6
            v[48:64:3] = 1e6
            v[80:96:4] = -1e6
        elif name == "gb_nonfinite":
            v[0], v[35], v[52] = np.nan, np.inf, -np.inf
        _put_floats(r, v)


GA_HBIAS = {5: 3e9, 100: -3e9, 200: 1.2e9, 300: 1e12}  # h-gate conditioning of these GRU_A units
# z- and r-gate conditioning of single units beyond 2^31 / 16256 = 132,104: _mm256_cvtps_epi32 gives INT_MIN there,
# one lane of a wave at a time (index into gru_a_dense_feature_bias: z [0, 384), r [384, 768))
GA_ZRBIAS = {7: 2e5, 250: -1e6, 384 + 150: -2e5, 384 + 64: 4e9}


@functools.lru_cache(maxsize=None)
def model(key: str) -> bytes:
    """The blob of 'int8' / 'fp32' / 'sat' (L.synthetic_model(1, variant)) or
    of an edited model '<name>/int8', '<name>/fp32'.  Every one passes
    L.validate_model."""
    name, _, var = key.rpartition("/")
    blob = L.synthetic_model(1, PLAIN[var][0], saturating=PLAIN[var][1])
    if name:
        recs = records(blob)
        if name.startswith("fc_"):
            _edit_fc(recs, name)
        elif name.startswith("gb_"):
            _edit_gb(recs, name)
        elif name == "ga_hbias":
            r = find(recs, "gru_a_dense_feature_bias")
            v = _floats(r)
            for u, x in GA_HBIAS.items():
                v[2 * NA + u] = x
            _put_floats(r, v)
        elif name == "ga_zrbias":
            r = find(recs, "gru_a_dense_feature_bias")
            v = _floats(r)
            for u, x in GA_ZRBIAS.items():
                v[u] = x
            _put_floats(r, v)
        else:
            raise KeyError(name)
        blob = join(recs)
        L.validate_model(blob)
    return blob


def variant_of(key: str) -> int:
    return PLAIN[key.rpartition("/")[2]][0]


def node_bound(key: str) -> float:
    """the largest |bias| + 2 sum|w| over the dual-FC nodes and channels: what the engine holds against the
    select-free tanh's domain"""
    recs = records(model(key))
    w = np.abs(_floats(find(recs, "dual_fc_weights")).astype(np.float64)).reshape(NLEVELS, 2, NB)
    b = np.abs(_floats(find(recs, "dual_fc_bias")).astype(np.float64)).reshape(2, NLEVELS)
    return float((b.T + 2 * w.sum(-1)).max())


# -- tail states -------------------------------------------------------------------------------

ALT = (-1.0) ** np.arange(16)
LAST_EXC = 77
EDGE8 = [32767.5, -32767.5, 32768, -32768, 0.49999997, -0.5, 1.5, 2.5]


# name -> the fields written over the stream's own: last_sig [16], sig_one (index, value) of last_sig, deemph,
# gru_b (index, value) of the GRU_B state, rng; last_exc becomes LAST_EXC in all of them
TAILS = {
    "sig_1e30": dict(last_sig=1e30 * ALT),
    "sig_3e38": dict(last_sig=3e38 * ALT),
    "sig_1e6": dict(last_sig=np.full(16, 1e6)),
    "sig_inf": dict(sig_one=(0, np.inf)),
    "sig_nan": dict(sig_one=(7, np.nan)),
    "sig_denorm": dict(last_sig=1e-42 * ALT, deemph=1e-42),
    "sig_edge": dict(last_sig=np.array(EDGE8 + EDGE8), deemph=32767.49),
    "de_3e38": dict(deemph=3e38),
    "de_m3e38": dict(deemph=-3e38),
    "de_1e6": dict(deemph=-1e6),
    "de_inf": dict(deemph=np.inf),
    "de_nan": dict(deemph=np.nan),
    "gb_nan": dict(gru_b=(3, np.nan)),
    "rng_zero": dict(rng=[0, 0, 0, 0]),
    "rng_ones": dict(rng=[0xFFFFFFFF] * 4),
}
# the tails that start finite and must come back to unclamped output within the run
RECOVERING = ["sig_1e30", "sig_3e38", "sig_1e6", "sig_denorm", "sig_edge", "de_3e38", "de_m3e38", "de_1e6"]


def apply_tail(name: str, last_sig, deemph, gru_b, rng):
    """(last_sig, deemph, last_exc, gru_b_state, rng) after the edit of TAILS[name]"""
    t = TAILS[name]
    sig = np.array(last_sig, np.float32)
    gb = np.array(gru_b, np.float32)
    if "last_sig" in t:
        sig = np.asarray(t["last_sig"]).astype(np.float32)
    if "sig_one" in t:
        sig[t["sig_one"][0]] = t["sig_one"][1]
    if "gru_b" in t:
        gb[t["gru_b"][0]] = t["gru_b"][1]
    de = F32(t["deemph"]) if "deemph" in t else F32(deemph)
    r = np.array(t["rng"], np.uint32) if "rng" in t else np.array(rng, np.uint32)
    return sig, de, LAST_EXC, gb, r


def edit_snapshot(name: str, snapshot: bytes) -> bytes:
    """a device stream's save_state bytes with the tail state of TAILS[name]"""
    s = np.frombuffer(snapshot, STATE).copy()
    sig, de, exc, gb, r = apply_tail(name, s[0]["last_sig"], s[0]["deemph_mem"], s[0]["gru_b_state"], s[0]["rng"])
    s[0]["last_sig"], s[0]["deemph_mem"], s[0]["last_exc"], s[0]["gru_b_state"], s[0]["rng"] = sig, de, exc, gb, r
    return s.tobytes()


# -- the cases -----------------------------------------------------------------------------------

NONFINITE = CF.NONFINITE + ["loud", "lpc_wide"]
# (model key, case): the case is a tail name, "plain" for an edited model, or "cond:<sequence>"
RUNS = ([(m, t) for m in PLAIN for t in TAILS] + [("%s/%s" % (e, m), "plain") for e in EDITED for m in VARIANTS] +
        [(m, "cond:" + s) for m in VARIANTS for s in NONFINITE])
_CASE_INDEX = {}
for _m, _c in RUNS:
    _CASE_INDEX.setdefault((_m.rpartition("/")[0], _c), len(_CASE_INDEX))


def case_index(key: str, case: str) -> int:
    """k of a case: the same for the int8 and fp32 run of it"""
    return _CASE_INDEX[(key.rpartition("/")[0], case)]


@functools.lru_cache(maxsize=None)
def features(key: str, case: str) -> np.ndarray:
    """[14, 20]: L.synthetic_features(k); a conditioning case's 12 edge frames first"""
    f = L.synthetic_features(case_index(key, case), NFRAMES)[:, :NF].astype(np.float32).copy()
    if case.startswith("cond:"):
        f[:CF.NFRAMES] = CF.features_of(case[5:])
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def teachers(key: str, case: str) -> dict:
    """frame -> int16 [160] with the teacher in the first `preload` samples; they differ per case"""
    k = case_index(key, case)
    rs = np.random.RandomState(SEED + k)
    t = np.arange(FRAME)
    a = np.where((t + k) % 2 == 0, 32767, -32768).astype(np.int16)
    b = np.rint(32767 * np.sin(0.3 * t + rs.uniform(0, 2 * np.pi))).astype(np.int16)
    out = {}
    for f, teach in ((5, a), (7, b)):
        buf = np.zeros(FRAME, np.int16)
        buf[:SCHEDULE[f][1]] = teach[:SCHEDULE[f][1]]
        buf.setflags(write=False)
        out[f] = buf
    return out


# -- the record of a frame ---------------------------------------------------------------------------

TAIL_WORDS = 22  # last_sig [16], deemph_mem, last_exc, rng [4]


def tail_words(last_sig, deemph, last_exc, rng) -> np.ndarray:
    """[22] uint32: the 17 floats with every NaN as 0x7FC00000 (as cond_frames.canon), last_exc, the kiss99 words"""
    fl = np.concatenate([np.asarray(last_sig, np.float32), np.array([deemph], np.float32)])
    w = fl.view(np.uint32).copy()
    w[np.isnan(fl)] = NAN
    return np.concatenate([w, np.array([last_exc], np.int32).view(np.uint32), np.asarray(rng, np.uint32)])


def canon_floats(a) -> np.ndarray:
    fl = np.ascontiguousarray(a, np.float32)
    w = fl.view(np.uint32).copy()
    w[np.isnan(fl)] = NAN
    return w


def state_digest(gru_a, gru_b) -> bytes:
    return hashlib.sha256(canon_floats(gru_a).tobytes() + canon_floats(gru_b).tobytes()).digest()


def snapshot_words(snapshot: bytes):
    """(tail words [22], gru_a_state words [384], gru_b_state words [16]) of a device stream's save_state bytes"""
    s = np.frombuffer(snapshot, STATE)[0]
    return (tail_words(s["last_sig"], s["deemph_mem"], int(s["last_exc"]), s["rng"]), canon_floats(s["gru_a_state"]),
            canon_floats(s["gru_b_state"]))


TAIL_FIELDS = [("last_sig", 0, 16), ("deemph_mem", 16, 17), ("last_exc", 17, 18), ("rng", 18, 22)]


# -- the oracle's run -----------------------------------------------------------------------------------

def oracle_run(key: str, case: str, kernels=None, avx2_build: bool = False, lib=None) -> dict:
    """The 14 frames of a case on the CPU oracle: pcm [14, 160] int16 (zeros
    past a short frame's N), tail [14, 22] uint32, gru_a [14, 384] and gru_b
    [14, 16] uint32 (NaN-canonical), digest [14, 32] uint8 of the two, logits
    [14, 160, 8] float32 and exc [14, 160] int32 (the trace; zeros past N and
    in the delay frames), nan_logits [14], clamped [14, 2] (samples the clamp
    put at +32767 / -32767, teacher-forced ones left out), ties [14, 8]
    (per tree level, the samples whose logit equals its threshold)."""
    o = O.Oracle(model(key), variant_of(key), kernels, avx2_build=avx2_build)
    feats, teach = features(key, case), teachers(key, case)
    out = dict(pcm=np.zeros((NFRAMES, FRAME), np.int16), tail=np.zeros((NFRAMES, TAIL_WORDS), np.uint32),
               gru_a=np.zeros((NFRAMES, NA), np.uint32), gru_b=np.zeros((NFRAMES, NB), np.uint32),
               digest=np.zeros((NFRAMES, 32), np.uint8), logits=np.zeros((NFRAMES, FRAME, 8), np.float32),
               exc=np.zeros((NFRAMES, FRAME), np.int32), nan_logits=np.zeros(NFRAMES, np.int32),
               clamped=np.zeros((NFRAMES, 2), np.int32), ties=np.zeros((NFRAMES, 8), np.int32))
    for f in range(NFRAMES):
        n, pre = SCHEDULE[f]
        pcm, lg, ex, rw = o.synthesize(feats[f], n, teach[f][:pre] if pre else None, trace=True)
        active = o.frame_count() > 2  # FEATURES_DELAY: the first two frames give zeros and leave the state alone
        out["pcm"][f, :n] = pcm
        if active:
            out["logits"][f, :n], out["exc"][f, :n] = lg, ex
            out["nan_logits"][f] = int(np.isnan(lg).sum())
            # nnet.c:178-184: level b's threshold is the table entry of byte b % 4 of draw b / 4
            thr = LT[(rw[:, np.arange(8) // 4] >> (8 * (np.arange(8) % 4)).astype(np.uint32)) & 0xFF]
            out["ties"][f] = (thr == lg).sum(0)
            out["clamped"][f] = [(pcm[pre:] == 32767).sum(), (pcm[pre:] == -32767).sum()]
        if f == TAIL_AFTER and case in TAILS:
            a, b = o.state()
            sig, de, exc, gb, r = apply_tail(case, *o.tail()[:2], b, o.tail()[3])
            o.set_tail(sig, de, exc, r)
            o.set_state(a, gb)
        a, b = o.state()
        out["tail"][f] = tail_words(*o.tail())
        out["gru_a"][f], out["gru_b"][f] = canon_floats(a), canon_floats(b)
        out["digest"][f] = np.frombuffer(state_digest(a, b), np.uint8)
    return out


# -- the fixture -------------------------------------------------------------------------------------

FIXTURE_KEYS = ("pcm", "tail", "digest", "nan_logits", "clamped", "ties")
_fix = None


def fixture() -> dict:
    """tests/golden/sampler_edge.npz, read-only: runs [R, 2] strings (model
    key, case), then per run pcm [R, 14, 160], tail [R, 14, 22], digest
    [R, 14, 32], nan_logits [R, 14], clamped [R, 14, 2], ties [R, 14, 8] -- all after each
    frame (the tail of frame 3 is the written one)."""
    global _fix
    if _fix is None:
        with np.load(GOLDEN) as g:
            _fix = {k: g[k] for k in g.files}
        for v in _fix.values():
            v.setflags(write=False)
        _fix["index"] = {(str(m), str(c)): r for r, (m, c) in enumerate(_fix["runs"])}
    return _fix


def expected(key: str, case: str) -> dict:
    fx = fixture()
    r = fx["index"][(key, case)]
    return {k: fx[k][r] for k in FIXTURE_KEYS}


def tail_diff(tag: str, frame, got: np.ndarray, exp: np.ndarray, what: str) -> list:
    """one line per differing field of two tail records"""
    out = []
    for name, lo, hi in TAIL_FIELDS:
        d = np.flatnonzero(got[lo:hi] != exp[lo:hi])
        if d.size:
            if name in ("last_sig", "deemph_mem"):
                show = lambda x: "%r (0x%08x)" % (float(np.uint32(x).view(np.float32)), x)  # noqa: E731
            else:
                show = lambda x: "0x%x" % x  # noqa: E731
            out.append("%s frame %s: %s differs from the %s at indices %s: got %s, expected %s"
                       % (tag, frame, name, what, d[:6].tolist(), show(got[lo + d[0]]), show(exp[lo + d[0]])))
    return out
