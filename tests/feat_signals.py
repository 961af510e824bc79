"""The edge-case signal set of the feature extractor: the generators
(tests/golden/make_enc_golden.py writes tests/golden/enc_features_edge.npz
from them through tests/enc_ref.py) and what the tests share: the fixture
loader, the per-frame state digest and the names of the state's fields.

The tests read PCM and answers from the fixture and never call a generator.
Every generator draws from its own np.random.RandomState (the frozen legacy
stream) with a fixed seed, so the maker is reproducible and a new signal
does not move the others.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import hashlib
import os

import numpy as np

FRAME = 160
NFRAMES = 24
N = NFRAMES * FRAME
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "enc_features_edge.npz")
SEED = 20261020

# name -> what it is there for
INT16 = [
    "chirp_up", "chirp_dn",                       # period 28 -> 270 and back: past both ends of the 32..256 search
    "p32", "p33", "p255", "p256", "p300",         # steady periods at and outside the search edges
    "stair_dn4", "stair_up4", "stair_dn3", "stair_dn8",  # the period moves by the Viterbi window's edge, inside it and beyond it
    "two40_80", "two50_150", "two45_90", "two64_128",    # sub-harmonic structure
    "noise_pulse", "step", "lsb", "dcmax", "dcmin", "nyq", "impulse", "fullnoise",
]
FLOAT32 = ["frac", "huge", "tiny", "tiny2", "tiny22", "sub40"]
NAMES = INT16 + FLOAT32

# EncRef.state_bytes(): (field, float32/int32 words), in order
STATE_FIELDS = [("analysis_mem", 160), ("exc_buf[160:]", 256), ("pitch_max_path[0]", 256), ("pitch_mem", 16),
                ("mem_preemph", 1), ("pitch_filt", 1), ("pitch_max_path_all", 1), ("best_i", 1)]
STATE_SIZE = 4 * sum(n for _, n in STATE_FIELDS)


def digest(state: bytes) -> bytes:
    return hashlib.sha256(state).digest()


def state_diff(a: bytes, b: bytes) -> list:
    """[(field, indices of the differing words)] of two state_bytes()."""
    x, y = np.frombuffer(a, np.uint32), np.frombuffer(b, np.uint32)
    assert x.size == y.size == STATE_SIZE // 4
    out, o = [], 0
    for name, n in STATE_FIELDS:
        d = np.flatnonzero(x[o:o + n] != y[o:o + n])
        if d.size:
            out.append((name, d.tolist()))
        o += n
    return out


def rng_of(name: str) -> np.random.RandomState:
    return np.random.RandomState(SEED + NAMES.index(name))


# -- generators ---------------------------------------------------------------

def resonate(x: np.ndarray) -> np.ndarray:
    """y[n] = x[n] + 1.2 y[n-1] - 0.72 y[n-2] in double (make_enc_golden.py's resonator)."""
    y = np.zeros(len(x) + 2)
    for n in range(len(x)):
        y[n + 2] = x[n] + 1.2 * y[n + 1] - 0.72 * y[n]
    return y[2:]


def pulses(period_at, n: int = N) -> np.ndarray:
    """Pulses of 6000; the one at sample p is followed by one at p + period_at(p)."""
    x = np.zeros(n)
    p = 0
    while p < n:
        x[p] += 6000.0
        p += max(1, int(round(period_at(p))))
    return x


def to_i16(y: np.ndarray) -> np.ndarray:
    return np.clip(np.rint(y), -32768, 32767).astype(np.int16)


def resonated(x: np.ndarray, rng) -> np.ndarray:
    """The resonated train plus uniform noise in [-20, 20], as int16."""
    return to_i16(resonate(x) + rng.randint(-20, 21, len(x)))


def stair(start: int, step: int, every: int):
    """The period moves by `step` every `every` samples, held inside [30, 280]."""
    return lambda p: min(280, max(30, start + step * (p // every)))


def make_int16(name: str) -> np.ndarray:
    rng = rng_of(name)
    if name == "chirp_up":
        return resonated(pulses(lambda p: 28 + (270 - 28) * p / N), rng)
    if name == "chirp_dn":
        return resonated(pulses(lambda p: 270 + (28 - 270) * p / N), rng)
    if name[0] == "p" and name[1:].isdigit():
        return resonated(pulses(lambda p: int(name[1:])), rng)
    if name.startswith("stair_"):
        start, step, every = {"stair_dn4": (200, -4, 80), "stair_up4": (60, 4, 80), "stair_dn3": (220, -3, 80),
                              "stair_dn8": (240, -8, 160)}[name]
        return resonated(pulses(stair(start, step, every)), rng)
    if name.startswith("two"):
        a, b = (int(v) for v in name[3:].split("_"))
        return resonated(pulses(lambda p: a) + pulses(lambda p: b), rng)
    if name == "noise_pulse":
        return to_i16(rng.randint(-3000, 3001, N) + 0.3 * resonate(pulses(lambda p: 75)))
    if name == "step":
        y = np.zeros(N)
        y[4 * FRAME:8 * FRAME] = rng.randint(-32768, 32768, 4 * FRAME)
        y[12 * FRAME:] = resonate(pulses(lambda p: 70, N - 12 * FRAME)) + rng.randint(-20, 21, N - 12 * FRAME)
        return to_i16(y)
    if name == "lsb":
        return rng.randint(-1, 2, N).astype(np.int16)
    if name == "dcmax":
        return np.full(N, 32767, np.int16)
    if name == "dcmin":
        return np.full(N, -32768, np.int16)
    if name == "nyq":
        return np.where(np.arange(N) % 2 == 0, 32767, -32768).astype(np.int16)
    if name == "impulse":
        y = np.zeros(N, np.int16)
        y[3 * FRAME] = 32767
        return y
    if name == "fullnoise":
        return rng.randint(-32768, 32768, N).astype(np.int16)
    raise KeyError(name)


def make_float32(name: str) -> np.ndarray:
    rng = rng_of(name)
    if name == "frac":  # not integer-valued
        return (0.37 * resonate(pulses(lambda p: 91)) + rng.uniform(-50, 50, N)).astype(np.float32)
    if name == "huge":  # outside int16
        return rng.uniform(-1e6, 1e6, N).astype(np.float32)
    if name == "tiny":
        # the Viterbi scores fw * xc (they go with scale^4) are subnormal, near
        # 1e-42, and pitch_max_path carries them across frames: at 1e-17 they
        # are still normal, at 1e-20 they are zero
        return (1e-19 * resonate(pulses(lambda p: 64))).astype(np.float32)
    if name == "tiny22":  # products of two samples are subnormal or zero; the scores underflow, every maximum ties
        return (1e-22 * resonate(pulses(lambda p: 64))).astype(np.float32)
    if name == "sub40":  # the samples themselves are subnormal, and most of the state with them
        return (1e-40 * resonate(pulses(lambda p: 64))).astype(np.float32)
    if name == "tiny2":  # frame energies next to the 1e-15 of process_single_frame
        return (1e-12 * resonate(pulses(lambda p: 64))).astype(np.float32)
    raise KeyError(name)


def make_all():
    """pcm_i16 [23, 24, 160] int16, pcm_f32 [6, 24, 160] float32."""
    return (np.stack([make_int16(n) for n in INT16]).reshape(len(INT16), NFRAMES, FRAME),
            np.stack([make_float32(n) for n in FLOAT32]).reshape(len(FLOAT32), NFRAMES, FRAME))


# -- the fixture ----------------------------------------------------------------

_fix = None


def fixture() -> dict:
    """The committed fixture, read-only: names, pcm_i16, pcm_f32, features
    [S, 24, 36], digests [S, 24, 32] uint8 (SHA-256 of state_bytes() after every
    frame), state [S, STATE_SIZE] uint8 (after the last frame)."""
    global _fix
    if _fix is None:
        with np.load(GOLDEN) as g:
            _fix = {k: g[k] for k in g.files}
        for v in _fix.values():
            v.setflags(write=False)
    return _fix


def pcm_of(name: str) -> np.ndarray:
    """[24, 160] of one signal, int16 or float32."""
    fx = fixture()
    k = NAMES.index(name)
    return fx["pcm_i16"][k] if k < len(INT16) else fx["pcm_f32"][k - len(INT16)]
