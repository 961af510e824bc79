"""The edge-case fixture of the feature extractor
(tests/golden/enc_features_edge.npz, signals of tests/feat_signals.py): what
the reference answers on it, that tests/enc_ref.py still reproduces it, and
the mutation table: one-line changes of enc_ref.py, of the kind a kernel
gets wrong, each of which the listed signals must notice."""
import types

import numpy as np
import pytest

import enc_ref as E
import feat_signals as FS

F = np.float32
needs_ref = pytest.mark.skipif(not E.have_ref(), reason="oracle/_ref (the reference's compiled kernels) not built")
S, NI, NFL = len(FS.NAMES), len(FS.INT16), len(FS.FLOAT32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pitch_feature(period2: int) -> np.float32:
    """features[18] for best[2] + best[3] = period2 (lpcnet_enc.c:865)."""
    return F(F(.01) * F(max(66, min(510, period2)) - 200))


def final_state(name: str):
    """(the float words, best_i) of a signal's state after the last frame."""
    st = FS.fixture()["state"][FS.NAMES.index(name)]
    return st[:-4].view(np.float32), int(st[-4:].view(np.int32)[0])


# -- fixture facts: no reference needed ----------------------------------------

def test_fixture_shapes_and_finite():
    fx = FS.fixture()
    assert list(fx["names"]) == FS.NAMES and len(set(FS.NAMES)) == S
    assert fx["pcm_i16"].shape == (NI, FS.NFRAMES, FS.FRAME) and fx["pcm_i16"].dtype == np.int16
    assert fx["pcm_f32"].shape == (NFL, FS.NFRAMES, FS.FRAME) and fx["pcm_f32"].dtype == np.float32
    assert fx["features"].shape == (S, FS.NFRAMES, E.NB_TOTAL_FEATURES) and fx["features"].dtype == np.float32
    assert fx["digests"].shape == (S, FS.NFRAMES, 32) and fx["digests"].dtype == np.uint8
    assert fx["state"].shape == (S, FS.STATE_SIZE) and fx["state"].dtype == np.uint8
    assert np.isfinite(fx["features"]).all() and np.isfinite(fx["pcm_f32"]).all()
    for k in range(S):
        assert np.isfinite(fx["state"][k, :-4].view(np.float32)).all(), FS.NAMES[k]
        # the last digest is that of the stored state
        assert FS.digest(fx["state"][k].tobytes()) == fx["digests"][k, -1].tobytes(), FS.NAMES[k]
    assert FS.NFRAMES == 24 and FS.STATE_SIZE == 4 * (160 + 256 + 256 + 16 + 4)


def test_fixture_signals_are_what_their_names_say():
    fx = FS.fixture()
    i16 = {n: fx["pcm_i16"][k].reshape(-1) for k, n in enumerate(FS.INT16)}
    f32 = {n: fx["pcm_f32"][k].reshape(-1) for k, n in enumerate(FS.FLOAT32)}
    assert (i16["dcmax"] == 32767).all() and (i16["dcmin"] == -32768).all()
    assert (i16["nyq"][0::2] == 32767).all() and (i16["nyq"][1::2] == -32768).all()
    assert np.flatnonzero(i16["impulse"]).tolist() == [3 * FS.FRAME] and i16["impulse"][3 * FS.FRAME] == 32767
    assert set(np.unique(i16["lsb"])) == {-1, 0, 1}
    assert i16["fullnoise"].min() < -32000 and i16["fullnoise"].max() > 32000
    st = fx["pcm_i16"][FS.INT16.index("step")]
    assert not st[:4].any() and not st[8:12].any() and np.abs(st[4:8]).max() > 32000 and st[12:].any()
    assert np.abs(f32["huge"]).max() > 9e5
    assert np.any(f32["frac"] != np.rint(f32["frac"]))
    for n, lo, hi in (("tiny2", 1e-9, 1e-7), ("tiny", 1e-16, 1e-14), ("tiny22", 1e-19, 1e-17)):
        assert lo < np.abs(f32[n]).max() < hi, n
    sub = f32["sub40"]
    # normal at the pulses, subnormal in the resonator's tails
    assert np.count_nonzero((np.abs(sub) < 2.0 ** -126) & (sub != 0)) > sub.size // 4
    assert np.count_nonzero(np.abs(sub) >= 2.0 ** -126) > sub.size // 4


def test_generators_reproduce_the_fixture_pcm():
    """The maker's input is reproducible: RandomState is a frozen stream."""
    i16, f32 = FS.make_all()
    fx = FS.fixture()
    assert i16.dtype == np.int16 and np.array_equal(i16, fx["pcm_i16"])
    assert f32.dtype == np.float32 and np.array_equal(bits(f32), bits(fx["pcm_f32"]))


def test_fixture_reaches_the_edges():
    """Stated on the reference's answers, so a trimmed set cannot pass."""
    fx = FS.fixture()
    f18 = bits(fx["features"][:, :, 18])
    # both clips of features[18]
    assert (f18 == bits(pitch_feature(66))).any() and (f18 == bits(pitch_feature(512))).any()
    assert pitch_feature(512) == pitch_feature(510) != pitch_feature(509) and pitch_feature(66) != pitch_feature(67)
    # both ends of the Viterbi states
    best = {final_state(n)[1] for n in FS.NAMES}
    assert 0 in best and E.NSTATES - 1 in best
    # the band-log clamps engage: a loud frame, then frames whose ceps[0] the clamps hold up
    c0 = fx["features"][FS.NAMES.index("dcmax"), :, 0]
    hot = np.flatnonzero(c0 > 17)
    assert hot.size and (c0[hot[0] + 1:] < -2).any()
    # subnormals in the carried state
    for n in ("tiny", "sub40"):
        w = final_state(n)[0]
        assert np.count_nonzero((np.abs(w) < 2.0 ** -126) & (w != 0)) >= 1, n
    # the range of ceps[0]: from the floor of silence to beyond int16
    assert fx["features"][:, :, 0].min() < -12 and fx["features"][:, :, 0].max() > 33


# -- the reference reproduces the fixture --------------------------------------

def run_signal(mod, name: str):
    """features [24, 36], digests [24] of bytes, the final state, by module `mod` (enc_ref or a mutant)."""
    r = mod.EncRef()
    feats, dig = [], []
    for frame in FS.pcm_of(name):
        feats.append(r.frame(frame))
        dig.append(FS.digest(r.state_bytes()))
    return np.stack(feats), dig, r.state_bytes()


def differs(mod, name: str) -> bool:
    """Whether `mod` changes a feature or a per-frame state digest of the signal."""
    k = FS.NAMES.index(name)
    fx = FS.fixture()
    r = mod.EncRef()
    for f, frame in enumerate(FS.pcm_of(name)):
        out = r.frame(frame)
        if not np.array_equal(bits(out), bits(fx["features"][k, f])) or FS.digest(r.state_bytes()) != fx["digests"][k, f].tobytes():
            return True
    return False


@needs_ref
@pytest.mark.parametrize("name", FS.NAMES)
def test_reference_reproduces_fixture(name):
    k = FS.NAMES.index(name)
    fx = FS.fixture()
    feats, dig, state = run_signal(E, name)
    for f in range(FS.NFRAMES):
        assert np.array_equal(bits(feats[f]), bits(fx["features"][k, f])), (name, f)
        assert dig[f] == fx["digests"][k, f].tobytes(), (name, f)
    assert state == fx["state"][k].tobytes(), FS.state_diff(state, fx["state"][k].tobytes())


# -- the mutation table ---------------------------------------------------------
# (name, text of enc_ref.py, its replacement, signals that must notice)

VIT_J = "for j in range(-4, 5):"
SUBH_LOOP = "for i in range(PITCH_MAX_PERIOD - 2 * PITCH_MIN_PERIOD):"
LOG_LINE = "ly = F(math.log10(1e-2 + float(Ex[i])))"
CLAMPS = "ly = _max16(F(logMax - F(8)), _max16(F(follow - F(2.5)), ly))"
MUTANTS = [
    # the Viterbi step (lpcnet_enc.c:831-842)
    ("vit_j_from_-3", VIT_J, "for j in range(-3, 5):", ["stair_dn4", "stair_dn8", "p256"]),
    ("vit_j_to_3", VIT_J, "for j in range(-4, 4):", ["stair_up4", "chirp_up"]),
    ("vit_upper_NS-1", "(idx + j < NS)", "(idx + j < NS - 1)", ["p33", "dcmax"]),
    ("vit_no_carried_max", "np.full(NS, F(self.pitch_max_path_all - F(6)), F)", "np.full(NS, F(F(0) - F(6)), F)",
     ["stair_dn4", "p32"]),
    # a tie inside the +-4 window: only the silence after a loud stretch flattens pitch_max_path into one
    ("vit_ge", "up = ok & (v > max_prev)", "up = ok & (v >= max_prev)", ["step"]),
    ("vit_penalty_in_double", "pen = F(F(F(.02) * F(abs(j))) * F(abs(j)))", "pen = F(.02 * abs(j) * abs(j))", ["p32", "chirp_up"]),
    ("vit_path_not_carried", "self.pitch_max_path[0] = self.pitch_max_path[1].copy()",
     "self.pitch_max_path[0] = np.zeros(PITCH_MAX_PERIOD, F)", ["tiny", "two45_90"]),
    ("argmax_tie_to_last", "if self.pitch_max_path[1][i] > max_path_all:", "if self.pitch_max_path[1][i] >= max_path_all:",
     ["impulse", "tiny22"]),
    ("clip_512", "min(510, ", "min(512, ", ["p256", "sub40"]),
    # the sub-harmonic check (:827-830)
    ("subh_191", SUBH_LOOP, "for i in range(PITCH_MAX_PERIOD - 2 * PITCH_MIN_PERIOD - 1):", ["lsb", "p33"]),
    ("subh_no_third_read", "r[(PITCH_MAX_PERIOD + i - 1) // 2])", "r[(PITCH_MAX_PERIOD + i) // 2])", ["chirp_up", "p255"]),
    ("subh_no_second_read", "r[(PITCH_MAX_PERIOD + i + 2) // 2])", "r[(PITCH_MAX_PERIOD + i) // 2])", ["chirp_dn", "fullnoise"]),
    ("subh_reads_scaled", SUBH_LOOP, "for i in reversed(range(PITCH_MAX_PERIOD - 2 * PITCH_MIN_PERIOD)):",
     ["chirp_up", "two40_80"]),
    # the 3x interpolation (:553-570)
    ("interp_from_5", "idx = np.arange(4, PITCH_MAX_PERIOD - 4)", "idx = np.arange(5, PITCH_MAX_PERIOD - 4)", ["chirp_dn", "p256"]),
    # the band logs (:514-520): only a constant at full scale reaches either clamp
    ("no_logmax_clamp", CLAMPS, "ly = _max16(F(follow - F(2.5)), ly)", ["dcmax", "dcmin"]),
    ("no_follow_clamp", CLAMPS, "ly = _max16(F(logMax - F(8)), ly)", ["dcmax", "dcmin"]),
    ("log_floor_in_float", LOG_LINE, "ly = F(math.log10(float(F(F(1e-2) + Ex[i]))))", ["p33", "impulse"]),
    ("log10_in_float", LOG_LINE, "ly = np.log10(F(1e-2 + float(Ex[i])))", ["tiny", "huge"]),
    # the frame weights (:822-823): only energies next to 1e-15 see the epsilon
    ("fws_eps_1e-14", "fws = F(1e-15)", "fws = F(1e-14)", ["tiny", "tiny2"]),
    ("fws_eps_1e-30", "fws = F(1e-15)", "fws = F(1e-30)", ["tiny22", "tiny2"]),
    # the running energy (:543-552)
    ("ener1_in_float", "ener1 += float(F(a * a))", "ener1 = float(F(F(ener1) + F(a * a)))", ["two40_80", "lsb"]),
    ("ener_sum_in_float", "ener = F(float(one_e0) + ener1)", "ener = F(one_e0 + F(ener1))", ["two50_150", "fullnoise"]),
    ("ener1_80_terms", "_inner_prod(e[off:off + FRAME_SIZE // 2 - 1], e[off:off + FRAME_SIZE // 2 - 1])",
     "_inner_prod(e[off:off + FRAME_SIZE // 2], e[off:off + FRAME_SIZE // 2])", ["p32", "nyq"]),
    # what crosses frames
    ("preemph_not_carried", "np.concatenate([[self.mem_preemph], ", "np.concatenate([[F(0)], ", ["dcmin", "frac"]),
    ("pitch_filt_not_carried", "np.concatenate([[self.pitch_filt], ", "np.concatenate([[F(0)], ", ["sub40", "huge"]),
    ("pitch_mem_not_carried", "np.concatenate([self.pitch_mem[::-1], aligned_in])",
     "np.concatenate([np.zeros(LPC_ORDER, F), aligned_in])", ["tiny22", "stair_dn3"]),
    ("exc_not_shifted", "self.exc_buf[:PITCH_MAX_PERIOD] = self.exc_buf[FRAME_SIZE:FRAME_SIZE + PITCH_MAX_PERIOD].copy()", "pass",
     ["impulse", "noise_pulse"]),
]

# Equivalent mutants, not in the table:
#  - interpolating up to index 250 instead of 251 (np.arange(4, PITCH_MAX_PERIOD - 5)):
#    the sub-harmonic check reads xc up to (256 + 191 + 2) // 2 = 224, the
#    Viterbi step and the backtrack up to state 223; nothing reads above 224.
#  - clipping the doubled period at 64 instead of 66: the 224 states make
#    2 * (256 - 223) = 66 the smallest sum.


def test_equivalent_mutants_stay_equivalent():
    top_read = (E.PITCH_MAX_PERIOD + (E.PITCH_MAX_PERIOD - 2 * E.PITCH_MIN_PERIOD - 1) + 2) // 2
    assert max(top_read, E.NSTATES - 1) < E.PITCH_MAX_PERIOD - 5  # index 251 is never read
    assert 2 * (E.PITCH_MAX_PERIOD - (E.NSTATES - 1)) == 66       # no sum lies below the lower clip
    assert 2 * E.PITCH_MAX_PERIOD == 512 > 510                    # the upper clip can engage (clip_512 is no equivalent)


def mutant(find: str, repl: str):
    """enc_ref.py with its single occurrence of `find` replaced, as a throw-away module."""
    with open(E.__file__.replace(".pyc", ".py")) as fh:
        src = fh.read()
    assert src.count(find) == 1, "%r occurs %d times in enc_ref.py" % (find, src.count(find))
    m = types.ModuleType("enc_ref_mutant")
    m.__file__ = E.__file__
    exec(compile(src.replace(find, repl), E.__file__, "exec"), m.__dict__)
    return m


@needs_ref
def test_unmutated_source_changes_nothing():
    m = mutant(VIT_J, VIT_J)
    assert m.EncRef is not E.EncRef
    for name in ("chirp_up", "dcmax", "tiny"):
        assert not differs(m, name), name


@needs_ref
@pytest.mark.parametrize("name,find,repl,signals", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutant_is_noticed(name, find, repl, signals):
    assert signals and set(signals) <= set(FS.NAMES)
    m = mutant(find, repl)
    blind = [s for s in signals if not differs(m, s)]
    assert not blind, "%s: not noticed on %s" % (name, blind)
