"""tests/burg_ref.py, the numpy restatement of burg_cepstral_analysis, against
tests/golden/burg_cepstrum.npz (the reference's compiled freq.c / burg.c on 33
signals) bit for bit, the fixture's coverage of the recursion's branches,
and, where oracle/_ref is built, against the compiled reference on random
frames.  Also: the library exports the Burg and predictor-row calls and the
Python mirror binds them (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest

import burg_ref as R
import feat_signals as FS
import lpcnet_amd as L

FX = R.fixture()
NEW_SYMBOLS = ["lpcnet_batch_burg_cepstrum", "lpcnet_batch_burg_cepstrum_float", "lpcnet_batch_burg_cepstrum_device",
               "lpcnet_batch_plc_rows_device", "lpcnet_batch_plc_update", "lpcnet_batch_plc_update_device"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def frame_errors(name, f, got, exp, what):
    """got, exp: (ceps, A, nrg, stop_order) of one frame; names the first stage that diverged."""
    out = []
    for h in range(2):
        if not np.array_equal(exp[3][h], got[3][h]):
            out.append("%s frame %d half %d: stop order %d, %s has %d" % (name, f, h, got[3][h], what, exp[3][h]))
        d = np.flatnonzero(bits(got[1][h]) != bits(exp[1][h]))
        if d.size:
            out.append("%s frame %d half %d: A%s differ from %s (the recursion)" % (name, f, h, d.tolist(), what))
        if bits(got[2])[h] != bits(exp[2])[h]:
            out.append("%s frame %d half %d: residual energy %r, %s has %r" % (name, f, h, got[2][h], what, exp[2][h]))
    d = np.flatnonzero(bits(got[0]) != bits(exp[0]))
    if d.size:
        out.append("%s frame %d: ceps%s differ from %s%s" % (name, f, d.tolist(), what,
                                                            "" if out else " (after the recursion: filter, FFT, bands, log, dct)"))
    return out


def test_fixture_shape():
    assert list(FX["names"]) == R.NAMES and len(R.NAMES) == 33
    assert FX["ceps"].shape == (33, FS.NFRAMES, 36) and FX["A"].shape == (33, FS.NFRAMES, 2, 16)
    assert FX["nrg"].shape == (33, FS.NFRAMES, 2) and FX["stop_order"].shape == (33, FS.NFRAMES, 2)
    assert FX["pcm_sine"].shape == (4, FS.NFRAMES, FS.FRAME) and FX["pcm_sine"].dtype == np.int16
    for k, n in enumerate(R.SINES):
        assert np.array_equal(FX["pcm_sine"][k].reshape(-1), R.make_sine(n)), n
    assert all(np.isfinite(FX[k]).all() for k in ("ceps", "A", "nrg"))


@pytest.mark.parametrize("name", R.NAMES)
def test_restatement_equals_fixture(name):
    s = R.NAMES.index(name)
    pcm = R.pcm_of(name)
    errors = []
    for f in range(FS.NFRAMES):
        errors += frame_errors(name, f, R.burg_frame(pcm[f]), (FX["ceps"][s, f], FX["A"][s, f], FX["nrg"][s, f], FX["stop_order"][s, f]),
                               "the fixture")
    assert not errors, "%d mismatches; the first: %s" % (len(errors), "\n".join(errors[:6]))


def test_fixture_covers_the_recursion():
    """Half-frames that stop at order 1, 2, 3 or 4, one of 6..9, 14, never
    (16), and with A all zero (0), from the signals expected to give them."""
    so = FX["stop_order"]

    def orders(*names):
        return set(np.unique(np.concatenate([so[R.NAMES.index(n)].reshape(-1) for n in names])).tolist())

    for n in ("dcmax", "dcmin", "nyq"):
        assert orders(n) == {1}, n
    assert orders("sine1") == {2}
    assert orders("sine2") & {3, 4}
    assert orders("sine3") & {6, 7, 8, 9}
    assert 14 in orders("sine5")
    assert 16 in orders(*R.NAMES)
    for n in ("impulse", "sub40", "step"):
        assert 0 in orders(n), n
    # stop_order is what the coefficients say: zeros after the clamped order
    A = FX["A"]
    for s in range(len(R.NAMES)):
        for f in range(FS.NFRAMES):
            for h in range(2):
                assert R.stop_from_A(A[s, f, h]) == so[s, f, h], (R.NAMES[s], f, h)


@pytest.mark.skipif(not R.have_ref(), reason="oracle/_ref (the reference's compiled kernels) not built")
@pytest.mark.parametrize("kind", ["int16", "float_1e-3", "float_1e5"])
def test_restatement_equals_compiled_reference(kind):
    rng = np.random.RandomState({"int16": 11, "float_1e-3": 12, "float_1e5": 13}[kind])
    errors = []
    for f in range(64):
        if kind == "int16":
            pcm = rng.randint(-32768, 32768, 160).astype(np.int16)
        else:
            pcm = (rng.randn(160) * (1e-3 if kind == "float_1e-3" else 1e5)).astype(np.float32)
        errors += frame_errors(kind, f, R.burg_frame(pcm), R.ref_frame(pcm), "the compiled reference")
    assert not errors, "%d mismatches; the first: %s" % (len(errors), "\n".join(errors[:6]))


def test_library_exports_and_mirror():
    """The C entry points are exported and the Python mirror binds them with
    their argument types; no device is touched."""
    raw = C.CDLL(L.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        fn = getattr(L.lib, name)
        assert fn.restype is C.c_int and fn.argtypes and fn.argtypes[0] is C.c_void_p, name
    assert L.lib.lpcnet_batch_burg_cepstrum_device.argtypes[3:5] == [C.c_int, C.c_int]
    assert L.lib.lpcnet_batch_plc_rows_device.argtypes[3:5] == [C.c_int, C.c_float]
    for m in ("burg_cepstrum", "burg_cepstrum_device", "plc_rows_device", "plc_update", "plc_update_device"):
        assert callable(getattr(L.LPCNetBatch, m)), m
    assert (L.BURG_CEPSTRUM, L.PLC_ROW_BURG, L.PLC_ROW_FEATURES) == (36, 1, 2)
    # argument errors are reported before any device call
    assert L.lib.lpcnet_batch_burg_cepstrum(None, None, None, None) == -1 and L.last_error()
    assert L.lib.lpcnet_batch_plc_rows_device(None, None, None, 0, 1.0, None) == -1 and L.last_error()
