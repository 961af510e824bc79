"""burg_cepstral_analysis on the device (burg_kernel.hip,
lpcnet_batch_burg_cepstrum*), the predictor's input rows
(lpcnet_batch_plc_rows_device) and the good-packet step
(lpcnet_batch_plc_update*) against tests/golden/burg_cepstrum.npz (the
reference's compiled freq.c / burg.c), tests/golden/enc_features_edge.npz and
tests/plc_ref.py.  Every comparison is bit for bit, on uint32 views.

The row and update calls take int16 PCM only, so they run on the 23 int16
signals of the extractor's set; its six float32 signals go through the two
kernels' float entries (here for Burg, tests/test_gpu_features_edge.py for the
extractor)."""
import ctypes as C

import numpy as np
import pytest

import burg_ref as R
import feat_signals as FS
import lpcnet_amd as L
import plc_ref as P

pytestmark = pytest.mark.gpu

NF, FRAME, NB, ROW = L.NB_FEATURES, L.FRAME_SIZE, L.BURG_CEPSTRUM, L.PLC_INPUTS
NFR = FS.NFRAMES
WG = 4  # streams per workgroup of burg_kernel (BURG_WG_STREAMS)
FX = R.fixture()
FFX = FS.fixture()
SENT = 0x7FC12345  # a NaN pattern no kernel produces
INT_NAMES = FS.INT16 + list(R.SINES)  # the 27 int16 signals
BOTH = L.PLC_ROW_BURG | L.PLC_ROW_FEATURES


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def sentinel(*shape):
    return np.full(shape, SENT, np.uint32).view(np.float32)


def want(name):
    return FX["ceps"][R.NAMES.index(name)]  # [24, 36]


def pcm_stack(names, dtype):
    """[S, 24, 160]: int16 signals convert to float exactly, as the reference's caller does."""
    return np.stack([np.asarray(R.pcm_of(n)).astype(dtype) for n in names])


def ceps_errors(name, f, got, exp, what="the fixture"):
    d = np.flatnonzero(bits(got) != bits(exp))
    return [] if not d.size else ["%s frame %d: ceps%s differ from %s (first: %r, expected %r)"
                                  % (name, f, d.tolist(), what, got[d[0]], exp[d[0]])]


def report(errors):
    assert not errors, "%d mismatches; the first: %s" % (len(errors), "\n".join(errors[:6]))


def run_host(names, dtype, blob=None, kernel=None, frames=range(NFR)):
    """ceps [S, len(frames), 36] of the single-frame host calls, one signal per stream."""
    S = len(names)
    pcm = pcm_stack(names, dtype)
    b = L.LPCNetBatch(S, 0)
    if blob is not None:
        b.load_model(blob)
        b.set_kernel(kernel)
    out = np.stack([b.burg_cepstrum(np.ascontiguousarray(pcm[:, f])) for f in frames], 1)
    b.close()
    return out


_all33 = None


def all33():
    """All 33 signals through the float entry on a batch with no model loaded, once."""
    global _all33
    if _all33 is None:
        _all33 = run_host(R.NAMES, np.float32)
        _all33.setflags(write=False)
    return _all33


# -- 1. the fixture ---------------------------------------------------------------

@pytest.mark.parametrize("name", R.NAMES)
def test_fixture_float_entry(require_gpu, name):
    """B = 33: eight whole workgroups and one of a single stream; no model."""
    assert len(R.NAMES) % WG != 0
    s = R.NAMES.index(name)
    report([e for f in range(NFR) for e in ceps_errors(name, f, all33()[s, f], want(name)[f])])


def test_fixture_short_entry(require_gpu):
    """The 27 int16 signals through the short entry (six workgroups and one of three)."""
    assert len(INT_NAMES) % WG != 0
    got = run_host(INT_NAMES, np.int16)
    report([e for s, n in enumerate(INT_NAMES) for f in range(NFR) for e in ceps_errors(n, f, got[s, f], want(n)[f])])


@pytest.mark.parametrize("names,dtype", [(["sine3"], np.int16), (["tiny22"], np.float32),
                                         (["dcmax", "sine1", "sine2", "impulse", "sine5"], np.int16),
                                         (["sub40", "huge", "nyq", "step", "frac"], np.float32)])
def test_small_batches(require_gpu, names, dtype):
    """B = 1 and B = 5: a partly filled first workgroup, a second one of one stream."""
    got = run_host(names, dtype)
    report([e for s, n in enumerate(names) for f in range(NFR) for e in ceps_errors(n, f, got[s, f], want(n)[f])])


def test_model_and_kernel_do_not_matter(require_gpu):
    """After load_model and set_kernel(1) the same 33 x 24 outputs as without a model."""
    got = run_host(R.NAMES, np.float32, L.synthetic_model(1, L.VARIANT_INT8), 1)
    assert np.array_equal(bits(got), bits(all33()))
    report([e for s, n in enumerate(R.NAMES) for f in range(NFR) for e in ceps_errors(n, f, got[s, f], want(n)[f])])


# -- 2. the active mask -------------------------------------------------------------

def test_active_mask(require_gpu):
    S = len(R.NAMES)
    pcm = pcm_stack(R.NAMES, np.float32)
    b = L.LPCNetBatch(S, 0)
    errors = []
    for f, phase in ((2, 0), (13, 1)):
        act = (np.arange(S) + phase) % 2 == 0
        out = sentinel(S, NB)
        b.burg_cepstrum(np.ascontiguousarray(pcm[:, f]), active=act.astype(np.uint8), out=out)
        for s, n in enumerate(R.NAMES):
            if act[s]:
                errors += ceps_errors(n, f, out[s], all33()[s, f], "the all-active run")
            elif not (bits(out[s]) == SENT).all():
                errors.append("%s frame %d: inactive, but its row lost the sentinel" % (n, f))
    b.close()
    report(errors)


# -- 3. the device form ---------------------------------------------------------------

@pytest.mark.parametrize("row,col", [(ROW, 0), (40, 4)])
def test_device_form(require_gpu, row, col):
    S, F0, NFD = len(INT_NAMES), 9, 3
    pcm = np.ascontiguousarray(np.moveaxis(pcm_stack(INT_NAMES, np.int16)[:, F0:F0 + NFD], 0, 1))  # [3, S, 160]
    b = L.LPCNetBatch(S, 0)
    d_pcm = b.device_alloc(pcm.nbytes)
    buf = sentinel(NFD, S, row)
    d_out = b.device_alloc(buf.nbytes)
    b.h2d(d_pcm, pcm)
    b.h2d(d_out, buf)
    b.burg_cepstrum_device(d_pcm, d_out, row, col, None, NFD)
    b.sync()
    got = np.zeros_like(buf)
    b.d2h(got, d_out)
    b.device_free(d_pcm)
    b.device_free(d_out)
    b.close()
    errors = []
    for s, n in enumerate(INT_NAMES):
        for f in range(NFD):
            errors += ceps_errors(n, F0 + f, got[f, s, col:col + NB], want(n)[F0 + f])
    rest = np.ones(row, bool)
    rest[col:col + NB] = False
    assert (bits(got)[:, :, rest] == SENT).all(), "a word outside columns %d..%d lost its sentinel" % (col, col + NB - 1)
    report(errors)


# -- 4. the predictor's input rows -------------------------------------------------------

class Rows:
    """A batch of the 23 int16 extractor signals with device PCM of all 24 frames and one row buffer."""

    def __init__(self):
        self.names = FS.INT16
        self.S = len(self.names)
        pcm = np.ascontiguousarray(np.moveaxis(FFX["pcm_i16"], 0, 1))  # [24, S, 160]
        self.b = L.LPCNetBatch(self.S, 0)
        self.d_pcm = self.b.device_alloc(pcm.nbytes)
        self.d_rows = self.b.device_alloc(self.S * ROW * 4)
        self.b.h2d(self.d_pcm, pcm)

    def rows(self, f, parts, flag):
        self.b.h2d(self.d_rows, sentinel(self.S, ROW))
        self.b.plc_rows_device(self.d_pcm + f * self.S * FRAME * 2, self.d_rows, parts, flag)
        self.b.sync()
        got = np.zeros((self.S, ROW), np.float32)
        self.b.d2h(got, self.d_rows)
        return got

    def states(self):
        return [self.b.features_save_state(s) for s in range(self.S)]

    def close(self):
        self.b.device_free(self.d_pcm)
        self.b.device_free(self.d_rows)
        self.b.close()


def row_errors(names, f, got, burg: bool, feat: bool, flag):
    errors = []
    for s, n in enumerate(names):
        k = FS.NAMES.index(n)
        exp = np.zeros(ROW, np.float32)
        if burg:
            exp[:NB] = want(n)[f]
        if feat:
            exp[NB:NB + NF] = FFX["features"][k, f, :NF]
        exp[ROW - 1] = flag
        d = np.flatnonzero(bits(got[s]) != bits(exp))
        if d.size:
            errors.append("%s frame %d: row columns %s differ (first: %r, expected %r)" % (n, f, d.tolist(), got[s][d[0]], exp[d[0]]))
    return errors


def test_rows_burg_and_features(require_gpu):
    r = Rows()
    errors = []
    for f in range(NFR):
        errors += row_errors(r.names, f, r.rows(f, BOTH, 1.0), True, True, 1.0)
        for s, n in enumerate(r.names):
            if FS.digest(r.b.features_save_state(s)) != FFX["digests"][FS.NAMES.index(n), f].tobytes():
                errors.append("%s frame %d: the analysis state's digest differs from the extractor fixture's" % (n, f))
    r.close()
    report(errors)


def test_rows_burg_only_keeps_the_analysis_state(require_gpu):
    r = Rows()
    errors = row_errors(r.names, 0, r.rows(0, BOTH, 1.0), True, True, 1.0)  # a state that is not the reset state
    before = r.states()
    for f in (0, 11):
        errors += row_errors(r.names, f, r.rows(f, L.PLC_ROW_BURG, 1.0), True, False, 1.0)
    assert r.states() == before
    r.close()
    report(errors)


def test_rows_features_only(require_gpu):
    r = Rows()
    errors = []
    for f in range(3):
        errors += row_errors(r.names, f, r.rows(f, L.PLC_ROW_FEATURES, -1.0), False, True, -1.0)
    r.close()
    report(errors)


def test_rows_active_mask(require_gpu):
    """Inactive streams keep their row, word for word, and their analysis state."""
    r = Rows()
    act = (np.arange(r.S) % 2 == 0).astype(np.uint8)
    d_act = r.b.device_alloc(r.S)
    r.b.h2d(d_act, act)
    before = r.states()
    r.b.h2d(r.d_rows, sentinel(r.S, ROW))
    r.b.plc_rows_device(r.d_pcm, r.d_rows, BOTH, 1.0, d_act)
    r.b.sync()
    got = np.zeros((r.S, ROW), np.float32)
    r.b.d2h(got, r.d_rows)
    after = r.states()
    on = [s for s in range(r.S) if act[s]]
    errors = row_errors([r.names[s] for s in on], 0, got[on], True, True, 1.0)
    for s in range(r.S):
        if not act[s]:
            assert (bits(got[s]) == SENT).all() and after[s] == before[s], r.names[s]
    r.b.device_free(d_act)
    r.close()
    report(errors)


# -- 5. the good-packet step -----------------------------------------------------------------

@pytest.mark.parametrize("form", ["host", "device"])
def test_plc_update(require_gpu, form):
    """B = 33 (the 23 int16 extractor signals, the first ten again), eight
    calls, alternating masks: a stream's k-th active call carries its frame k.
    Output and predictor state equal PlcRef on rows assembled on the host from
    the two fixtures, and plc_predict on those rows."""
    blob = L.synthetic_model(1, L.VARIANT_INT8, plc_small=True)
    names = [FS.INT16[s % len(FS.INT16)] for s in range(33)]
    B = len(names)
    idx = [FS.NAMES.index(n) for n in names]
    b = L.LPCNetBatch(B, 0, blob)
    b2 = L.LPCNetBatch(B, 0, blob)
    refs = [P.PlcRef(blob) for _ in range(B)]
    if form == "device":
        d_pcm, d_out, d_act = b.device_alloc(B * FRAME * 2), b.device_alloc(B * NF * 4), b.device_alloc(B)
    done = np.zeros(B, np.int64)
    errors = []
    for c in range(8):
        act = (np.arange(B) + c) % 2 == 0
        pcm = np.ascontiguousarray(FFX["pcm_i16"][idx, done])
        pcm[~act] = -12345
        rows = np.zeros((B, ROW), np.float32)
        for s in range(B):
            rows[s, :NB] = want(names[s])[done[s]]
            rows[s, NB:NB + NF] = FFX["features"][idx[s], done[s], :NF]
            rows[s, ROW - 1] = 1
        out = sentinel(B, NF)
        if form == "host":
            b.plc_update(pcm, active=act, out=out)
        else:
            b.h2d(d_pcm, pcm)
            b.h2d(d_out, out)
            b.h2d(d_act, act.astype(np.uint8))
            b.plc_update_device(d_pcm, d_out, d_act)
            b.sync()
            b.d2h(out, d_out)
        out2 = sentinel(B, NF)
        b2.plc_predict(rows, active=act, out=out2)
        for s in range(B):
            if act[s]:
                exp = refs[s].predict(rows[s])
                if not np.array_equal(bits(out[s]), bits(exp)):
                    errors.append("%s call %d (frame %d): output differs from PlcRef" % (names[s], c, done[s]))
                if not np.array_equal(bits(out[s]), bits(out2[s])):
                    errors.append("%s call %d (frame %d): output differs from plc_predict on the host-assembled row" % (names[s], c, done[s]))
            elif not (bits(out[s]) == SENT).all():
                errors.append("%s call %d: inactive, but its output row lost the sentinel" % (names[s], c))
            st = b.plc_save_state(s)
            if st != refs[s].save() or st != b2.plc_save_state(s):
                errors.append("%s call %d: predictor state differs from PlcRef's or plc_predict's" % (names[s], c))
        done += act
    assert (done == 4).all()
    if form == "device":
        for p in (d_pcm, d_out, d_act):
            b.device_free(p)
    b.close()
    b2.close()
    report(errors)


# -- 6. arguments -------------------------------------------------------------------------------

def refused(rc):
    assert rc == -1 and L.last_error(), "accepted, or refused without a reason"


def test_arguments(require_gpu):
    B = 5
    lib = L.lib
    b = L.LPCNetBatch(B, 0, L.synthetic_model(1, L.VARIANT_INT8, plc_small=True))
    nop = L.LPCNetBatch(B, 0, L.synthetic_model(1, L.VARIANT_INT8))  # no PLC records
    pcm = np.zeros((B, FRAME), np.int16)
    pcm_f = np.zeros((B, FRAME), np.float32)
    ceps, out = sentinel(B, NB), sentinel(B, NF)
    dev = sentinel(3 * B * ROW)
    d_pcm = b.device_alloc(3 * B * FRAME * 2)
    d_buf = b.device_alloc(dev.nbytes)
    n_pcm, n_buf = nop.device_alloc(B * FRAME * 2), nop.device_alloc(B * NF * 4)
    b.h2d(d_pcm, np.zeros((3, B, FRAME), np.int16))
    b.h2d(d_buf, dev)
    nop.h2d(n_pcm, pcm)
    nop.h2d(n_buf, out)
    h, p, f, c, o = b._b, pcm.ctypes.data, pcm_f.ctypes.data, ceps.ctypes.data, out.ctypes.data
    for rc in (lambda: lib.lpcnet_batch_burg_cepstrum(h, None, c, None), lambda: lib.lpcnet_batch_burg_cepstrum(h, p, None, None),
               lambda: lib.lpcnet_batch_burg_cepstrum(None, p, c, None),
               lambda: lib.lpcnet_batch_burg_cepstrum_float(h, None, c, None), lambda: lib.lpcnet_batch_burg_cepstrum_float(h, f, None, None),
               lambda: lib.lpcnet_batch_burg_cepstrum_device(h, None, d_buf, ROW, 0, None, 1),
               lambda: lib.lpcnet_batch_burg_cepstrum_device(h, d_pcm, None, ROW, 0, None, 1),
               lambda: lib.lpcnet_batch_burg_cepstrum_device(None, d_pcm, d_buf, ROW, 0, None, 1),
               lambda: lib.lpcnet_batch_burg_cepstrum_device(h, d_pcm, d_buf, 40, 5, None, 1),   # row < col + 36
               lambda: lib.lpcnet_batch_burg_cepstrum_device(h, d_pcm, d_buf, NB - 1, 0, None, 1),
               lambda: lib.lpcnet_batch_burg_cepstrum_device(h, d_pcm, d_buf, ROW, -1, None, 1),  # col < 0
               lambda: lib.lpcnet_batch_burg_cepstrum_device(h, d_pcm, d_buf, ROW, 0, None, -1),  # nframes < 0
               lambda: lib.lpcnet_batch_plc_rows_device(h, None, d_buf, BOTH, 1.0, None),
               lambda: lib.lpcnet_batch_plc_rows_device(h, d_pcm, None, BOTH, 1.0, None),
               lambda: lib.lpcnet_batch_plc_rows_device(None, d_pcm, d_buf, BOTH, 1.0, None),
               lambda: lib.lpcnet_batch_plc_rows_device(h, d_pcm, d_buf, 0, 1.0, None),           # parts outside 1..3
               lambda: lib.lpcnet_batch_plc_rows_device(h, d_pcm, d_buf, 4, 1.0, None),
               lambda: lib.lpcnet_batch_plc_rows_device(h, d_pcm, d_buf, -1, 1.0, None),
               lambda: lib.lpcnet_batch_plc_update(h, None, o, None), lambda: lib.lpcnet_batch_plc_update(h, p, None, None),
               lambda: lib.lpcnet_batch_plc_update(None, p, o, None),
               lambda: lib.lpcnet_batch_plc_update_device(h, None, d_buf, None),
               lambda: lib.lpcnet_batch_plc_update_device(h, d_pcm, None, None),
               lambda: lib.lpcnet_batch_plc_update_device(None, d_pcm, d_buf, None)):
        refused(rc())
    # a model without PLC records: the update refuses with the reason, the rows do not need it
    for rc in (lambda: lib.lpcnet_batch_plc_update(nop._b, p, o, None), lambda: lib.lpcnet_batch_plc_update_device(nop._b, n_pcm, n_buf, None)):
        refused(rc())
        assert "no PLC records" in L.last_error()
    b.sync()
    nop.sync()
    got = np.zeros_like(dev)
    b.d2h(got, d_buf)
    got_n = np.zeros_like(out)
    nop.d2h(got_n, n_buf)
    for a in (ceps, out, got, got_n):
        assert (bits(a) == SENT).all(), "a refused call wrote to its output"
    assert b.kernel_ms(6)[1] == 0
    b.burg_cepstrum_device(d_pcm, d_buf, ROW, 0, None, 0)  # nframes = 0: nothing to do, no error
    for q in (d_pcm, d_buf):
        b.device_free(q)
    for q in (n_pcm, n_buf):
        nop.device_free(q)
    b.close()
    nop.close()


# -- 7. the timer ----------------------------------------------------------------------------------

def test_timer(require_gpu):
    B = 6
    b = L.LPCNetBatch(B, 0)
    pcm = np.ascontiguousarray(pcm_stack(["sine2"] * B, np.int16)[:, :2].transpose(1, 0, 2))  # [2, B, 160]
    d_pcm, d_out, d_rows = b.device_alloc(pcm.nbytes), b.device_alloc(2 * B * NB * 4), b.device_alloc(B * ROW * 4)
    b.h2d(d_pcm, pcm)

    def calls():
        for _ in range(3):
            b.burg_cepstrum(pcm[0])
        b.burg_cepstrum_device(d_pcm, d_out, NB, 0, None, 2)
        b.plc_rows_device(d_pcm, d_rows, BOTH, 1.0)
        b.plc_rows_device(d_pcm, d_rows, L.PLC_ROW_FEATURES, 1.0)  # no Burg launch
        b.sync()

    b.reset_timers(1)
    calls()
    ms, n = b.kernel_ms(6)
    assert n == 6 and ms > 0 and b.kernel_frames(6) == 6
    assert b.kernel_ms(3)[1] == 2
    b.reset_timers(0)
    calls()
    assert b.kernel_ms(6)[1] == 0 and b.kernel_ms(3)[1] == 0
    assert L.lib.lpcnet_batch_kernel_ms(b._b, 7, None) == -1
    for q in (d_pcm, d_out, d_rows):
        b.device_free(q)
    b.close()
