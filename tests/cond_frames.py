"""The edge-case feature frames of the conditioning network
(run_frame_network, lpcnet.c:82-120): the generators
(tests/golden/make_cond_golden.py writes tests/golden/cond_edge.npz from them
through the CPU oracle), the two model variants that make the pitch row and
subnormal products visible, and what the tests share: the fixture loader, the
per-frame record and its digest, and a diff helper that names sequence, frame,
field and indices.

The tests read features and answers from the fixture and never call a
generator.  Every sequence is NFRAMES frames x 20 float32 features and draws
from its own np.random.RandomState (the frozen legacy stream) with a fixed
seed, so the maker is reproducible and a new sequence does not move the
others.  "Base frame" is frame 5 of lpcnet_mi355x_synthetic_features(0).
TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import functools
import hashlib
import math
import os

import numpy as np

import lpcnet_amd as L
from test_ingest import find, join, records

NFRAMES = 12
NF = 20
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cond_edge.npz")
SEED = 20261021
F32 = np.float32
INT_MIN = -(1 << 31)

# Finite class: the reference's conditioning and LPC are finite in every frame
# (tests/test_cond_frames_ref.py asserts it: a condition of membership).
FINITE = [
    "zeros",          # all-zero frames: conditioning from the biases alone
    "neg_zeros",      # -0.0 everywhere: sign of zero through the chains and tanh
    "const",          # the base frame 12 times: the conv windows fill up and settle
    "impulse",        # zeros except frame 4: conv1 carries it over frames 4..6, conv2 over 4..8, then it is gone
    "alt_sign",       # base frame x (-1)^f: every window mixes signs
    "pitch_edges0",   # f18 on the float32 neighbours (-2..+2) of (k - 100.1) / 50: k = 33, 34 and two of 100's
    "pitch_edges1",   # ... the rest of 100's, 176 and four of 254's
    "pitch_edges2",   # ... the last of 254's, 255, 256 and -1.5: at and beyond the upper clamp
    "pitch_edges3",   # -5, 3.2, 10 (beyond both clamps), 0, and the true floor boundaries of rows 34, 100, 176, 255
    "pitch_forms",    # f18 at which each plausible wrong form of the pitch expression picks another row
    "loud",           # c0 = 40, bands x 10: saturated tanh in every layer, band power near the top of float
    "scale_lo",       # base frame x 10^(f - 11): 1e-11 .. 1: windows mixing small magnitudes
    "tiny",           # x 1e-30: products underflow to subnormals and zero
    "subnormal",      # x 1e-42: the inputs themselves are subnormal
    "corr_edges",     # f19 in {+-0.5, +-10}
    "lpc_wide",       # cepstra N(0, 8): band powers over the whole finite range, redrawn until every LPC is finite
]
# Non-finite class: through the frame network only.  Where the reference is
# NaN the device must be NaN (x86's 0xFFC00000 and the GPU's 0x7FC00000 both
# count), everything else matches bit for bit, and the fixture pins how many
# values per frame are NaN.
NONFINITE = [
    # f18 = +-1e10: the double lies outside int (x86 cvttsd2si: INT_MIN, hence row 33 for either sign).  On the plain
    # models conv1's sums reach 1e9, where the reference's Pade tanh is inf * 0 = NaN; on pitch_only every value is finite
    "pitch_huge",
    "scale_ramp",     # base frame x 10^(f - 6): windows mixing 1e-6 .. 1e5; from 1e2 on the band power overflows (LPC NaN)
    "nan_band",       # one NaN in band 3 of frame 5
    "inf_c0",         # c0 = +inf in frame 4, -inf in frame 8
    "inf_pitch",      # f18 = +inf, -inf, NaN in frames 3, 6, 9
    "lpc_overflow",   # c0 = 200 in frames 3..5: band power inf (10^(0.2357 c0) leaves float above c0 = 163), LPC NaN,
                      # conditioning finite
    "max_float",      # band 7 = 3e38 in frame 5
]
NAMES = FINITE + NONFINITE
# the sequences the two model variants run
VARIANT_SEQS = ["pitch_edges0", "pitch_edges1", "pitch_edges2", "pitch_edges3", "pitch_forms", "pitch_huge", "zeros", "tiny",
                "subnormal"]

SUBNORMAL_SEQS = ["zeros", "neg_zeros", "scale_lo", "tiny", "subnormal"]

# name -> (variant, (LPC_GAMMA, FEATURES_DELAY, END2END) or None for the defaults, sequences)
MODELS = {
    "int8": (L.VARIANT_INT8, None, NAMES),
    "fp32": (L.VARIANT_FP32, None, NAMES),
    "pitch_only": (L.VARIANT_INT8, None, VARIANT_SEQS),   # conv1 sees the pitch embedding alone
    "zero_bias": (L.VARIANT_INT8, None, VARIANT_SEQS),    # the frame network's biases zeroed
    # zero biases and no pitch embedding in conv1: with the embedding row (values near 0.1) in every conv1 sum, zero
    # biases alone still swallow subnormal products; here they survive to the outputs
    "features_only": (L.VARIANT_INT8, None, SUBNORMAL_SEQS),
    "g092_d3": (L.VARIANT_INT8, (0.92, 3, 0), NAMES),
    "e2e_g09_d1": (L.VARIANT_INT8, (0.9, 1, 1), NAMES),
}
RUNS = [(m, s) for m, (_, _, seqs) in MODELS.items() for s in seqs]

# one frame's outputs and what it leaves behind: (field, 32-bit words), in the record's order
FIELDS = [("gru_a_cond", 1152), ("gru_b_cond", 48), ("lpc", 16), ("conv1_mem", 168), ("conv2_mem", 256), ("frame_count", 1)]
WORDS = sum(n for _, n in FIELDS)
OFFSET = {}
_o = 0
for _n, _k in FIELDS:
    OFFSET[_n] = (_o, _o + _k)
    _o += _k
NAN = 0x7FC00000
FIN, COND, CONV_K = 84, 128, 3


# -- models ---------------------------------------------------------------------

def _floats(rec) -> np.ndarray:
    size = int(np.frombuffer(bytes(rec[1][12:16]), np.int32)[0])
    return np.frombuffer(bytes(rec[2][:size]), np.float32).copy()


def _put_floats(rec, v: np.ndarray) -> None:
    data = np.ascontiguousarray(v, np.float32).tobytes()
    assert len(data) == int(np.frombuffer(bytes(rec[1][12:16]), np.int32)[0])
    rec[2][:len(data)] = data


VARIANTS = ("pitch_only", "zero_bias", "features_only")
BIASES = ["feature_conv1_bias", "feature_conv2_bias", "feature_dense1_bias", "feature_dense2_bias",
          "gru_a_dense_feature_bias", "gru_b_dense_feature_bias"]


@functools.lru_cache(maxsize=None)
def model(name: str) -> bytes:
    """The blob of a model of MODELS (cached).  pitch_only, zero_bias and
    features_only edit records of L.synthetic_model(1, int8) and pass
    L.validate_model."""
    variant = MODELS[name][0]
    blob = L.synthetic_model(1, variant)
    if name == "pitch_only":
        # conv1's weights are [tap][input][row]: zero the rows of the 20 features in all three taps
        recs = records(blob)
        r = find(recs, "feature_conv1_weights")
        w = _floats(r).reshape(CONV_K, FIN, COND)
        w[:, :NF, :] = 0
        _put_floats(r, w)
        blob = join(recs)
    elif name in ("zero_bias", "features_only"):
        recs = records(blob)
        if name == "features_only":
            r = find(recs, "feature_conv1_weights")
            w = _floats(r).reshape(CONV_K, FIN, COND)
            w[:, NF:, :] = 0
            _put_floats(r, w)
        for b in BIASES:
            r = find(recs, b)
            _put_floats(r, np.zeros_like(_floats(r)))
        blob = join(recs)
    if name in VARIANTS:
        L.validate_model(blob)
    return blob


# -- the pitch expression and its plausible wrong forms ---------------------------

def _clamp(p: int) -> int:
    return 255 if p > 255 else (33 if p < 33 else p)


def _to_int(v: float) -> int:
    """(int) of a double on x86 (cvttsd2si): out of range or NaN gives INT_MIN."""
    return int(v) if v == v and -2147483648.0 <= v < 2147483648.0 else INT_MIN


def pitch_ref(f18) -> int:
    """lpcnet.c:93-94: (int)floor(.1 + 50*features[18] + 100) -- a float
    product, then double adds -- clamped to [33, 255]."""
    p = F32(50) * F32(f18)
    return _clamp(_to_int(math.floor((0.1 + float(p)) + 100.0)))


def pitch_all_float(f18) -> int:
    v = F32(F32(F32(0.1) + F32(50) * F32(f18)) + F32(100))
    return _clamp(_to_int(math.floor(float(v))))


def pitch_all_double(f18) -> int:
    return _clamp(_to_int(math.floor((0.1 + 50.0 * float(F32(f18))) + 100.0)))


def pitch_no_tenth(f18) -> int:
    return _clamp(_to_int(math.floor(float(F32(50) * F32(f18)) + 100.0)))


def pitch_rint(f18) -> int:
    return _clamp(_to_int(float(np.rint((0.1 + float(F32(50) * F32(f18))) + 100.0))))


WRONG_FORMS = {"all_float": pitch_all_float, "all_double": pitch_all_double, "no_tenth": pitch_no_tenth, "rint": pitch_rint}
DECODER_RANGE = (-1.34, 3.1)  # features[18] of the 1.6 kb/s decoder: 0.02 (p - 100), p in [33, 255]


def _step(x: np.float32, n: int) -> np.float32:
    """the float32 n steps above (n > 0) or below x"""
    for _ in range(abs(n)):
        x = np.nextafter(F32(x), F32(np.inf if n > 0 else -np.inf), dtype=np.float32)
    return F32(x)


def _edge(k: int) -> np.float32:
    return F32((k - 100.1) / 50)


def _floor_boundary(k: int):
    """(the largest float32 whose row is k - 1, the smallest whose row is k): bisection on the float32 order."""
    lo, hi = F32((k - 101) / 50.0), F32((k - 99.5) / 50.0)
    assert pitch_ref(lo) < k <= pitch_ref(hi)
    # the bit pattern as an integer that grows with the value; the map is its own inverse
    key = lambda i: i if i >= 0 else INT_MIN - i  # noqa: E731
    val = lambda m: np.int32(key(m)).view(np.float32)  # noqa: E731
    a, b = key(int(lo.view(np.int32))), key(int(hi.view(np.int32)))
    while b - a > 1:
        m = (a + b) // 2
        if pitch_ref(val(m)) >= k:
            b = m
        else:
            a = m
    return val(a), val(b)


def pitch_edge_values() -> np.ndarray:
    """the 48 f18 values of pitch_edges0..3"""
    v = [_step(_edge(k), d) for k in (33, 34, 100, 176, 254, 255, 256) for d in (-2, -1, 0, 1, 2)]
    v += [F32(-1.5), F32(-5), F32(3.2), F32(10), F32(0)]
    for k in (34, 100, 176, 255):
        v += list(_floor_boundary(k))
    assert len(v) == 4 * NFRAMES
    return np.array(v, np.float32)


def pitch_form_values() -> np.ndarray:
    """Three f18 per wrong form at which it picks another row than the
    reference, after clamping: the first, the middle and the last separating
    value among the float32 neighbours (-3..+3) of (k - 100.1) / 50 and of
    (k - 100) / 50, k = 34..255, that lie inside the decoder's range.  A form
    that cannot be separated fails the assertion."""
    cand = [_step(F32(c), d) for k in range(34, 256) for c in ((k - 100.1) / 50, (k - 100) / 50.0) for d in range(-3, 4)]
    cand = [c for c in cand if DECODER_RANGE[0] <= c <= DECODER_RANGE[1]]
    out = []
    for name, form in WRONG_FORMS.items():
        sep = [c for c in cand if form(c) != pitch_ref(c)]
        assert len(sep) >= 3, "the pitch form %s cannot be separated from the reference's" % name
        out += [sep[0], sep[len(sep) // 2], sep[-1]]
    assert len(out) == NFRAMES
    return np.array(out, np.float32)


def form_separation(f18: np.ndarray) -> dict:
    """form -> the values of f18 at which it picks another row than pitch_ref"""
    return {n: [float(v) for v in f18 if fn(v) != pitch_ref(v)] for n, fn in WRONG_FORMS.items()}


# -- generators -------------------------------------------------------------------

def rng_of(name: str) -> np.random.RandomState:
    return np.random.RandomState(SEED + NAMES.index(name))


def base_frame() -> np.ndarray:
    return L.synthetic_features(0, 6)[5, :NF].astype(np.float32).copy()


def make(name: str, lpc_finite=None) -> np.ndarray:
    """[NFRAMES, 20] float32.  lpc_finite(frames) -> bool is the redraw
    condition of lpc_wide (the maker passes the reference's)."""
    base = base_frame()
    const = np.tile(base, (NFRAMES, 1))
    rng = rng_of(name)
    if name == "zeros":
        return np.zeros((NFRAMES, NF), np.float32)
    if name == "neg_zeros":
        return np.full((NFRAMES, NF), -0.0, np.float32)
    if name == "const":
        return const
    if name == "impulse":
        x = np.zeros((NFRAMES, NF), np.float32)
        x[4] = base
        return x
    if name == "alt_sign":
        return (const * ((-1.0) ** np.arange(NFRAMES))[:, None]).astype(np.float32)
    if name.startswith("pitch_edges"):
        k = int(name[-1])
        const[:, 18] = pitch_edge_values()[k * NFRAMES:(k + 1) * NFRAMES]
        return const
    if name == "pitch_forms":
        const[:, 18] = pitch_form_values()
        return const
    if name == "pitch_huge":
        # + - - + ...: the last frame and frame 4 (the last of a 5-frame run) are +1e10, where x86 and a saturating cast part
        const[:, 18] = np.where(np.isin(np.arange(NFRAMES) % 4, (0, 3)), 1e10, -1e10).astype(np.float32)
        return const
    if name == "loud":
        const[:, 0] = 40
        const[:, 1:18] *= F32(10)
        return const
    if name == "scale_lo":
        return (const.astype(np.float64) * 10.0 ** (np.arange(NFRAMES) - 11.0)[:, None]).astype(np.float32)
    if name == "scale_ramp":
        return (const.astype(np.float64) * 10.0 ** (np.arange(NFRAMES) - 6.0)[:, None]).astype(np.float32)
    if name == "tiny":
        return (const.astype(np.float64) * 1e-30).astype(np.float32)
    if name == "subnormal":
        return (const.astype(np.float64) * 1e-42).astype(np.float32)
    if name == "corr_edges":
        const[:, 19] = np.tile(np.array([0.5, -0.5, 10, -10], np.float32), NFRAMES // 4)
        return const
    if name == "lpc_wide":
        for _ in range(1000):
            const[:, :18] = rng.normal(0, 8, (NFRAMES, 18)).astype(np.float32)
            if lpc_finite is None or lpc_finite(const):
                return const
        raise AssertionError("lpc_wide: no finite draw")
    if name == "nan_band":
        const[5, 3] = np.nan
        return const
    if name == "inf_c0":
        const[4, 0], const[8, 0] = np.inf, -np.inf
        return const
    if name == "inf_pitch":
        const[3, 18], const[6, 18], const[9, 18] = np.inf, -np.inf, np.nan
        return const
    if name == "lpc_overflow":
        const[3:6, 0] = 200
        return const
    if name == "max_float":
        const[5, 7] = 3e38
        return const
    raise KeyError(name)


# -- records, digests, diffs --------------------------------------------------------

def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def canon(words: np.ndarray) -> np.ndarray:
    """The record with every NaN as 0x7FC00000 (x86 makes 0xFFC00000, the GPU
    0x7FC00000): "NaN where the reference is NaN, bit-equal elsewhere" is
    equality of canonical records.  frame_count, the last word, is an int."""
    w = np.array(words, np.uint32)
    f = w[..., :WORDS - 1]
    f[np.isnan(f.view(np.float32))] = NAN
    return w


def record(a, b, lpc, c1, c2, frame_count: int) -> np.ndarray:
    """One frame's canonical record [WORDS] uint32, in the order of FIELDS."""
    return canon(np.concatenate([bits(a), bits(b), bits(lpc), bits(c1), bits(c2), np.array([frame_count], np.uint32)]))


def oracle_record(o) -> np.ndarray:
    """The record of an oracle_lib.Oracle after a frame."""
    a, b, lpc = o.frame()
    c1, c2 = o.conv_mem()
    return record(a, b, lpc, c1, c2, o.frame_count())


# StreamState (lpcnet_engine.h), as lpcnet_batch_save_state returns it
STATE = np.dtype([("gru_a_state", "<f4", 384), ("gru_a_cond", "<f4", 1152), ("gru_b_cond", "<f4", 48),
                  ("gru_b_state", "<f4", 16), ("last_sig", "<f4", 16), ("lpc", "<f4", 16),
                  ("old_lpc", "<f4", (4, 16)), ("conv1_mem", "<f4", 168), ("conv2_mem", "<f4", 256),
                  ("deemph_mem", "<f4"), ("last_exc", "<i4"), ("frame_count", "<i4"), ("rng", "<u4", 4),
                  ("vq_mem", "<f4", 18), ("pad", "<i4", 3)])


def state_record(snapshot: bytes) -> np.ndarray:
    """The record of a device stream from its save_state bytes."""
    s = np.frombuffer(snapshot, STATE)[0]
    return record(s["gru_a_cond"], s["gru_b_cond"], s["lpc"], s["conv1_mem"], s["conv2_mem"], int(s["frame_count"]))


def digest(rec: np.ndarray) -> bytes:
    return hashlib.sha256(np.ascontiguousarray(rec, np.uint32).tobytes()).digest()


def nan_count(rec: np.ndarray) -> int:
    return int(np.isnan(np.ascontiguousarray(rec[:WORDS - 1]).view(np.float32)).sum())


def field(rec: np.ndarray, name: str) -> np.ndarray:
    lo, hi = OFFSET[name]
    return rec[..., lo:hi]


def diff(seq: str, frame, got: np.ndarray, exp: np.ndarray, what: str = "reference", fields=None) -> list:
    """One line per differing field of two records: sequence, frame, field,
    the first differing indices and the first pair of values."""
    out = []
    for name, _ in FIELDS:
        if fields is not None and name not in fields:
            continue
        g, e = field(got, name), field(exp, name)
        d = np.flatnonzero(g != e)
        if d.size:
            show = (lambda x: int(x)) if name == "frame_count" else (lambda x: "%r (0x%08x)" % (float(np.uint32(x).view(np.float32)), x))
            out.append("%s frame %s: %s differs from the %s at %d indices, first %s: got %s, expected %s"
                       % (seq, frame, name, what, d.size, d[:6].tolist(), show(g[d[0]]), show(e[d[0]])))
    return out


# -- the fixture ------------------------------------------------------------------

_fix = None


def fixture() -> dict:
    """The committed fixture, read-only: names [S], features [S, 12, 20],
    models [M], runs [R, 2] (model, sequence), digests [R, 12, 32] uint8
    (SHA-256 of the canonical record after every frame), gru_b_cond
    [R, 12, 48] and lpc [R, 12, 16] uint32, nan_count [R, 12], last [R, WORDS]
    uint32 (the whole record of the last frame)."""
    global _fix
    if _fix is None:
        with np.load(GOLDEN) as g:
            _fix = {k: g[k] for k in g.files}
        for v in _fix.values():
            v.setflags(write=False)
        _fix["run_index"] = {(str(_fix["models"][m]), str(_fix["names"][s])): r for r, (m, s) in enumerate(_fix["runs"])}
    return _fix


def features_of(name: str) -> np.ndarray:
    """[12, 20] float32 of one sequence, from the fixture."""
    fx = fixture()
    return fx["features"][list(fx["names"]).index(name)]


def run_of(model_name: str, seq: str) -> int:
    return fixture()["run_index"][(model_name, seq)]


def fixture_diff(model_name: str, seq: str, frame: int, rec: np.ndarray) -> list:
    """What a frame's record disagrees with in the fixture: the stored fields,
    the NaN count, the digest (and the whole record in the last frame)."""
    fx = fixture()
    r = run_of(model_name, seq)
    tag = "%s/%s" % (model_name, seq)
    out = []
    for name in ("gru_b_cond", "lpc"):
        d = np.flatnonzero(field(rec, name) != fx[name][r, frame])
        if d.size:
            out.append("%s frame %d: %s differs from the fixture at indices %s" % (tag, frame, name, d[:6].tolist()))
    if nan_count(rec) != fx["nan_count"][r, frame]:
        out.append("%s frame %d: %d NaN values, the fixture has %d" % (tag, frame, nan_count(rec), fx["nan_count"][r, frame]))
    if frame == NFRAMES - 1:
        out += diff(tag, frame, rec, fx["last"][r], "fixture")
    if digest(rec) != fx["digests"][r, frame].tobytes():
        out.append("%s frame %d: the record's digest differs from the fixture's" % (tag, frame))
    return out
