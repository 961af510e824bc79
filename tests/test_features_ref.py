"""The CPU reference of the feature extractor (tests/enc_ref.py) against the
committed fixture tests/golden/enc_features.npz, the pitch facts the fixture's
signals were chosen for, and the host-only argument checks of the
lpcnet_batch_*features* calls (no device needed)."""
import ctypes as C

import numpy as np
import pytest

import enc_ref as E
import lpcnet_amd as L

F = np.float32
needs_ref = pytest.mark.skipif(not E.have_ref(), reason="oracle/_ref (the reference's compiled kernels) not built")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pitch_feature(period2: int) -> np.float32:
    """features[18] for best[2] + best[3] = period2 (lpcnet_enc.c:865)."""
    return F(F(.01) * F(max(66, min(510, period2)) - 200))


def test_fixture_shape_and_finite():
    pcm, feats = E.golden()
    assert pcm.shape == (5, 12, E.FRAME_SIZE) and pcm.dtype == np.int16
    assert feats.shape == (5, 12, E.NB_TOTAL_FEATURES) and feats.dtype == np.float32
    assert np.isfinite(feats).all()
    assert list(np.load(E.GOLDEN)["names"]) == E.SIGNALS
    assert np.abs(pcm[4]).min() == 32767 and not pcm[2].any()


def test_fixture_pitch_facts():
    """The periodic signals settle on their period (two half-frame lags:
    twice the period) with a pitch correlation near 1 (features[19] near .5);
    silence keeps the all-tied answer on every frame."""
    _, feats = E.golden()
    for s, period in ((0, 80), (1, 57), (4, 100)):
        assert np.array_equal(bits(feats[s, -4:, 18]), bits(np.full(4, pitch_feature(2 * period)))), E.SIGNALS[s]
        assert np.all(np.abs(feats[s, -4:, 19] - .5) < .01), E.SIGNALS[s]
    # silence: best_i stays 0 in both half-frames, best[2] + best[3] = 512 -> clipped to 510; no correlation
    assert np.array_equal(bits(feats[2, :, 18]), bits(np.full(12, pitch_feature(512))))
    assert pitch_feature(512) == F(3.1)
    assert np.array_equal(bits(feats[2, :, 19]), bits(np.full(12, F(-.5))))
    # noise has no stable pitch and a low correlation
    assert np.all(feats[3, :, 19] < 0)


@needs_ref
def test_reference_reproduces_fixture():
    """enc_ref on the reference's compiled kernels, bit for bit; the strict >
    of the Viterbi search is exercised: every first half-frame, and silence
    throughout, has all 224 maxima tied."""
    pcm, feats = E.golden()
    for s in range(len(pcm)):
        r = E.EncRef()
        for f in range(pcm.shape[1]):
            out = r.frame(pcm[s, f])
            assert np.array_equal(bits(out), bits(feats[s, f])), (E.SIGNALS[s], f)
            if f == 0:
                assert r.tied[0] == E.NSTATES
            if s == 2:
                assert r.tied == [E.NSTATES, E.NSTATES] and r.period == 512
        assert len(r.state_bytes()) == L.lib.lpcnet_batch_features_state_size(None)


@needs_ref
def test_reference_float_input():
    """Floats that hold the int16 values give the same features (the
    reference converts short to float first, lpcnet_plc.c:251)."""
    pcm, feats = E.golden()
    r = E.EncRef()
    for f in range(3):
        assert np.array_equal(bits(r.frame(pcm[3, f].astype(np.float32))), bits(feats[3, f]))


@needs_ref
def test_half_window_formula():
    """The engine builds half_window from dump_lpcnet_tables.c's formula; the
    reference ships the printed table: the same floats."""
    import math
    mine = np.array([math.sin(.5 * math.pi * math.sin(.5 * math.pi * (i + .5) / 160) * math.sin(.5 * math.pi * (i + .5) / 160))
                     for i in range(160)]).astype(np.float32)
    assert np.array_equal(bits(mine), bits(E.half_window()))


# -- host-only argument checks: refused before any device is touched ----------

def test_state_size_positive_and_stable():
    n = L.lib.lpcnet_batch_features_state_size(None)
    assert n > 0 and n % 16 == 0
    assert n == L.lib.lpcnet_batch_features_state_size(None)
    # analysis_mem, exc tail, pitch_max_path[0], pitch_mem, three scalars and best_i
    assert n == 4 * (160 + 256 + 256 + 16 + 4)


@pytest.mark.parametrize("row", [0, 18, 19, 21, 35, 37, -20])
def test_device_form_rejects_other_rows(row):
    buf = (C.c_float * 64)()
    assert L.lib.lpcnet_batch_compute_features_device(None, C.addressof(buf), C.addressof(buf), row, None, 1) == -1
    assert "row" in L.last_error()


def test_device_form_accepts_both_rows_then_needs_a_batch():
    buf = (C.c_float * 64)()
    for row in (L.NB_FEATURES, L.NB_TOTAL_FEATURES):
        assert L.lib.lpcnet_batch_compute_features_device(None, C.addressof(buf), C.addressof(buf), row, None, 1) == -1
        assert "null batch" in L.last_error()
    assert L.lib.lpcnet_batch_compute_features_device(None, C.addressof(buf), C.addressof(buf), 20, None, -1) == -1
    assert "nframes" in L.last_error()


def test_bad_stream_index_and_null_arguments():
    buf = C.create_string_buffer(L.lib.lpcnet_batch_features_state_size(None))
    assert L.lib.lpcnet_batch_features_reset(None, -2) == -1
    assert "no such stream" in L.last_error()
    assert L.lib.lpcnet_batch_features_save_state(None, -1, buf) == -1
    assert "no such stream" in L.last_error()
    assert L.lib.lpcnet_batch_features_restore_state(None, -1, buf) == -1
    assert "no such stream" in L.last_error()
    assert L.lib.lpcnet_batch_features_save_state(None, 0, None) == -1
    assert L.lib.lpcnet_batch_compute_features(None, None, None, None) == -1
    assert L.lib.lpcnet_batch_compute_features_float(None, None, None, None) == -1


def test_restore_rejects_a_best_i_outside_the_search():
    """best_i indexes the Viterbi rows on the device: a snapshot with one
    outside [0, 224) is refused on the host."""
    n = L.lib.lpcnet_batch_features_state_size(None)
    for bad in (-1, E.NSTATES, 1 << 20):
        st = np.zeros(n // 4, np.int32)
        st[-1] = bad
        assert L.lib.lpcnet_batch_features_restore_state(None, 0, st.ctypes.data) == -1
        assert "best_i" in L.last_error()
