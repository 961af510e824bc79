"""The feature extractor on the device (feat_kernel.hip) on the edge-case
signals of tests/feat_signals.py against tests/golden/enc_features_edge.npz:
the features of every frame on uint32 views, the analysis state after every
frame by its SHA-256, the final state byte for byte, and, where oracle/_ref
is built, live tests/enc_ref.py.  A mismatch names the signal, the frame and
the feature indices or the state's fields (the layout of
EncRef.state_bytes)."""
import numpy as np
import pytest

import enc_ref as E
import feat_signals as FS
import lpcnet_amd as L

pytestmark = pytest.mark.gpu

NF, NTF, FRAME = L.NB_FEATURES, L.NB_TOTAL_FEATURES, L.FRAME_SIZE
NFR = FS.NFRAMES
WG = 4  # streams per workgroup of feat_kernel (FEAT_WG_STREAMS)
FX = FS.fixture()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def want(name: str):
    """The fixture's (features [24, 36], digests [24, 32], final state bytes) of a signal."""
    k = FS.NAMES.index(name)
    return FX["features"][k], FX["digests"][k], FX["state"][k].tobytes()


def feature_errors(name: str, f: int, got: np.ndarray, exp: np.ndarray, what: str = "fixture") -> list:
    d = np.flatnonzero(bits(got) != bits(exp[:got.size]))
    return [] if not d.size else ["%s frame %d: features %s differ from the %s (first: %r, expected %r)"
                                  % (name, f, d.tolist(), what, got[d[0]], exp[d[0]])]


class Run:
    """One signal per stream through 24 single-frame calls: feats [S, 24, 36],
    the state of every stream after every frame, and what disagreed with the
    fixture or with live enc_ref, per signal."""

    def __init__(self, names, live_ref: bool = True):
        self.names = list(names)
        S = len(self.names)
        pcm = np.stack([FS.pcm_of(n) for n in self.names])  # [S, 24, 160]
        refs = [E.EncRef() for _ in range(S)] if live_ref and E.have_ref() else None
        self.errors = {n: [] for n in self.names}
        self.feats = np.zeros((S, NFR, NTF), np.float32)
        self.states = [[None] * NFR for _ in range(S)]
        b = L.LPCNetBatch(S, 0)
        for f in range(NFR):
            out = b.compute_features(np.ascontiguousarray(pcm[:, f]))
            assert out.shape == (S, NTF)
            self.feats[:, f] = out
            for s, n in enumerate(self.names):
                st = self.states[s][f] = b.features_save_state(s)
                exp_f, exp_d, exp_st = want(n)
                err = self.errors[n]
                err += feature_errors(n, f, out[s], exp_f[f])
                if FS.digest(st) != exp_d[f].tobytes():
                    err.append("%s frame %d: the state's digest differs from the fixture's" % (n, f))
                if f == NFR - 1 and st != exp_st:
                    err.append("%s: final state differs from the fixture in %s" % (n, FS.state_diff(st, exp_st)))
                if refs:
                    err += feature_errors(n, f, out[s], refs[s].frame(pcm[s, f]), "live enc_ref")
                    if st != refs[s].state_bytes():
                        err.append("%s frame %d: state differs from live enc_ref in %s"
                                   % (n, f, FS.state_diff(st, refs[s].state_bytes())))
        b.close()
        self.feats.setflags(write=False)


_runs = {}


def run_of(kind: str) -> Run:
    """The int16 set (23 streams: five whole workgroups and one of three) and
    the float32 set, each in a batch of its own, computed once."""
    if kind not in _runs:
        _runs[kind] = Run(FS.INT16 if kind == "int16" else FS.FLOAT32)
    return _runs[kind]


def report(errors: list):
    assert not errors, "%d mismatches; the first: %s" % (len(errors), "\n".join(errors[:6]))


@pytest.mark.parametrize("name", FS.INT16)
def test_int16_set(require_gpu, name):
    assert len(FS.INT16) % WG != 0 and len(FS.INT16) > 5 * WG
    report(run_of("int16").errors[name])


@pytest.mark.parametrize("name", FS.FLOAT32)
def test_float_set(require_gpu, name):
    r = run_of("float")
    assert FS.pcm_of(name).dtype == np.float32
    report(r.errors[name])


@pytest.mark.parametrize("rot", [1, WG + 1])
def test_placement(require_gpu, rot):
    """The int16 set rotated by one stream and by a workgroup and one: every
    signal changes wave slot and workgroup, and with the slot the lane of
    wave 0 that runs its Levinson recursion.  Same answers per signal."""
    S = len(FS.INT16)
    names = [FS.INT16[(s - rot) % S] for s in range(S)]
    assert all(names.index(n) % WG != k % WG for k, n in enumerate(FS.INT16))
    assert rot == 1 or all(names.index(n) // WG != k // WG for k, n in enumerate(FS.INT16))
    r = Run(names, live_ref=False)
    base = run_of("int16")
    errors = []
    for s, n in enumerate(names):
        errors += r.errors[n]
        k = FS.INT16.index(n)
        if not np.array_equal(bits(r.feats[s]), bits(base.feats[k])):
            errors.append("%s: stream %d differs from stream %d of the unrotated batch" % (n, s, k))
        if r.states[s] != base.states[k]:
            f = next(f for f in range(NFR) if r.states[s][f] != base.states[k][f])
            errors.append("%s: state at stream %d differs from stream %d's from frame %d in %s"
                          % (n, s, k, f, FS.state_diff(r.states[s][f], base.states[k][f])))
    report(errors)


@pytest.mark.parametrize("row", [NTF, NF])
def test_device_form(require_gpu, row):
    """All 24 frames of the int16 set in one compute_features_device call: the
    single-frame results (the first `row` of each) and the same final states."""
    S = len(FS.INT16)
    base = run_of("int16")
    pcm = np.ascontiguousarray(np.moveaxis(FX["pcm_i16"], 0, 1))  # [24, S, 160]
    b = L.LPCNetBatch(S, 0)
    d_pcm = b.device_alloc(pcm.nbytes)
    d_feat = b.device_alloc(NFR * S * row * 4)
    b.h2d(d_pcm, pcm)
    b.compute_features_device(d_pcm, d_feat, row, None, NFR)
    b.sync()
    got = np.zeros((NFR, S, row), np.float32)
    b.d2h(got, d_feat)
    states = [b.features_save_state(s) for s in range(S)]
    b.device_free(d_pcm)
    b.device_free(d_feat)
    b.close()
    errors = []
    for s, n in enumerate(FS.INT16):
        for f in range(NFR):
            errors += feature_errors(n, f, got[f, s], want(n)[0][f])
            errors += feature_errors(n, f, got[f, s], base.feats[s, f], "single-frame call")
        if states[s] != want(n)[2]:
            errors.append("%s: final state differs from the fixture in %s" % (n, FS.state_diff(states[s], want(n)[2])))
        if states[s] != base.states[s][-1]:
            errors.append("%s: final state differs from the single-frame calls' in %s"
                          % (n, FS.state_diff(states[s], base.states[s][-1])))
    report(errors)


def test_masked_interleave(require_gpu):
    """One workgroup: chirp_up active on even calls, dcmax on odd ones, beside
    impulse (silence but for one sample) and fullnoise on every call.  Each
    sees its fixture frames in order; a masked stream keeps its state and its
    output row, whatever PCM it is handed."""
    names = ["chirp_up", "dcmax", "impulse", "fullnoise"]
    assert len(names) == WG
    pcm = np.stack([FS.pcm_of(n) for n in names])
    b = L.LPCNetBatch(WG, 0)
    done = np.zeros(WG, np.int64)
    out = np.full((WG, NTF), np.float32(-77.25))
    errors = []
    for call in range(2 * NFR):
        act = np.array([call % 2 == 0, call % 2 == 1, call < NFR, call >= NFR])
        p = np.ascontiguousarray(pcm[np.arange(WG), np.minimum(done, NFR - 1)])
        p[~act] = -12345
        before = [b.features_save_state(s) for s in range(WG)]
        prev = out.copy()
        b.compute_features(p, active=act.astype(np.uint8), out=out)
        for s, n in enumerate(names):
            st = b.features_save_state(s)
            if act[s]:
                f = int(done[s])
                errors += feature_errors(n, f, out[s], want(n)[0][f])
                if FS.digest(st) != want(n)[1][f].tobytes():
                    errors.append("%s frame %d (call %d): the state's digest differs from the fixture's" % (n, f, call))
            else:
                errors += feature_errors(n, int(done[s]), out[s], prev[s], "row it held while masked (call %d)" % call)
                if st != before[s]:
                    errors.append("%s: masked in call %d, state moved in %s" % (n, call, FS.state_diff(st, before[s])))
        done += act
    assert (done == NFR).all()
    for s, n in enumerate(names):
        st = b.features_save_state(s)
        if st != want(n)[2]:
            errors.append("%s: final state differs from the fixture in %s" % (n, FS.state_diff(st, want(n)[2])))
    b.close()
    report(errors)
