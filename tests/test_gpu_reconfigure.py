"""Reconfiguration between frames.  The other GPU modules configure a batch
once, before frame 0; here lpcnet_batch_set_kernel, _set_rcp_table and
_set_model_constants are called between frames of a running batch, so that

* every sample kernel has to hand a complete StreamState to the next one
  (mf_kernel and its split form, mf2_kernel, mfw_kernel with 2 and 3 groups
  and its split form, fp_kernel and its long form, each followed and preceded
  by the lockstep kernel on the same streams);
* a setter must not undo another setter: a change of the kernel mode or of
  the rcpps table that moves the batch across the wide kernel's plan class
  re-plans the register tables from the kept blob, and the constants set
  with lpcnet_batch_set_model_constants have to survive that;
* the batch's own feature buffer (host-visible VRAM on large-BAR devices)
  feeds the per-frame path of small batches and teacher-forced calls.

The reference is always the CPU oracle (one Oracle per stream) or a golden
fixture.  Tolerance 0: integer PCM identical, floats
bit-equal, snapshots byte-equal."""
import os

import numpy as np
import pytest

import lpcnet_amd as L
import oracle_lib as O

pytestmark = pytest.mark.gpu

DEFAULTS = (1.0, 2, 0)
# StreamState (lpcnet_engine.h), field by field: a snapshot that differs names its fields
STATE = np.dtype([("gru_a_state", "<f4", 384), ("gru_a_cond", "<f4", 1152), ("gru_b_cond", "<f4", 48),
                  ("gru_b_state", "<f4", 16), ("last_sig", "<f4", 16), ("lpc", "<f4", 16),
                  ("old_lpc", "<f4", (4, 16)), ("conv1_mem", "<f4", 168), ("conv2_mem", "<f4", 256),
                  ("deemph_mem", "<f4"), ("last_exc", "<i4"), ("frame_count", "<i4"), ("rng", "<u4", 4),
                  ("vq_mem", "<f4", 18), ("pad", "<i4", 3)])


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def feats(stream, nframes):
    return L.synthetic_features(stream, nframes)[:, :20]


def state_diff(x: bytes, y: bytes):
    """Names of the StreamState fields in which two snapshots differ."""
    a, b = np.frombuffer(x, STATE)[0], np.frombuffer(y, STATE)[0]
    return [n for n in STATE.names if a[n].tobytes() != b[n].tobytes()]


class _Frames:
    """lpcnet_batch_synthesize_frames of allf[f0:f1] ([F, B, 20]), enqueued
    only; result() waits and returns the PCM [F, B, 160]."""

    def __init__(self, b, allf, f0, f1):
        part = np.ascontiguousarray(allf[f0:f1], np.float32)
        self.b, self.shape = b, part.shape[:2]
        self.df = b.device_alloc(part.nbytes)
        self.dp = b.device_alloc(self.shape[0] * self.shape[1] * 160 * 2)
        b.h2d(self.df, part)
        b.synthesize_frames(part, self.df, self.dp, self.shape[0])

    def result(self):
        self.b.sync()
        got = np.zeros(self.shape + (160,), np.int16)
        self.b.d2h(got, self.dp)
        self.b.device_free(self.df)
        self.b.device_free(self.dp)
        return got


def check_info_constants(b, c):
    i = b.info()
    assert (np.float32(i.lpc_gamma), i.features_delay, i.end2end) == (np.float32(c[0]), int(c[1]), int(c[2])), \
        (i.lpc_gamma, i.features_delay, i.end2end)


def expected(blob, variant, allf, constants=None, switch=None):
    """Oracle PCM [F, B, 160] of features allf [F, B, 20], one Oracle per
    stream, and the oracles; switch = (frame, constants) changes the
    constants before that frame."""
    F, B = allf.shape[:2]
    refs = [O.Oracle(blob, variant, constants=constants) for _ in range(B)]
    out = np.zeros((F, B, 160), np.int16)
    for f in range(F):
        for s in range(B):
            if switch is not None and f == switch[0]:
                refs[s].set_constants(*switch[1])
            out[f, s] = refs[s].synthesize(allf[f, s])
    return out, refs


def assert_guard(exp, other, frames, what):
    """Vacuity guard, CPU only: in `frames` every stream's expected PCM
    differs from what the error under test would give."""
    for s in range(exp.shape[1]):
        assert (exp[frames, s] != other[frames, s]).any(), (what, s)


# model, B, environment, (quad_path, kernel name or its prefix, long_rows) of the automatic kernel
HANDOVER = [
    pytest.param(0, False, 3, {}, (4, "mf_kernel<", 0), id="mf"),
    pytest.param(0, False, 8, {"LPCNET_MFW": "1", "LPCNET_MFW_G": "2"}, (7, "mfw_kernel<true, 2, false>", 0), id="mfw2"),
    pytest.param(0, False, 12, {"LPCNET_MFW": "1", "LPCNET_MFW_G": "3"}, (7, "mfw_kernel<true, 3, false>", 0), id="mfw3"),
    pytest.param(0, False, 8, {"LPCNET_MF2": "1", "LPCNET_MFW": "0"}, (6, "mf2_kernel<", 0), id="mf2"),
    pytest.param(0, True, 3, {}, (4, "mf_kernel<", 1), id="mf-split"),
    pytest.param(0, True, 8, {"LPCNET_MFW": "1"}, (7, "mfw_kernel<true, 2, true>", 1), id="mfw-split"),
    pytest.param(1, False, 3, {}, (5, "fp_kernel<", 0), id="fp"),
    pytest.param(1, True, 3, {}, (5, "fp_kernel<", 1), id="fp-long"),
]


@pytest.mark.parametrize("variant,skewed,B,env,auto", HANDOVER)
def test_kernel_handover_between_frames(require_gpu, monkeypatch, variant, skewed, B, env, auto):
    """One batch, ten frames, the sample kernel switched between frames:
    frames 0-2 per frame on the automatic kernel (0-1 are the silent
    FEATURES_DELAY frames), 3-4 per frame on the lockstep kernel, 5-8 in one
    device-resident lpcnet_batch_synthesize_frames call on the automatic
    kernel again (a multi-frame sample launch on the int8 fast kernels),
    frame 9 on the lockstep kernel through the batch's own feature buffer.
    info() pins the kernel of each segment.  Every stream's PCM on every
    frame and its final GRU states equal one Oracle per stream, and every
    stream's snapshot is byte-equal to that of a batch that ran the same
    entry points without any set_kernel call.  On the mfw rows each
    set_kernel also moves the plan class and re-plans the register tables."""
    for k in ("LPCNET_MFW", "LPCNET_MFW_G", "LPCNET_MF2"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    F = 10
    blob = L.synthetic_model(1, variant, skewed=skewed)
    allf = np.ascontiguousarray(np.stack([feats(s, F) for s in range(B)], 1))
    exp, refs = expected(blob, variant, allf)
    assert not exp[:2].any() and np.abs(exp[3:].astype(np.float64)).mean() > 100

    def on_auto(b):
        i = b.info()
        assert (i.quad_path, i.long_rows) == (auto[0], auto[2]), (i.quad_path, i.long_rows)
        # a full template instance where the case names one, else the kernel's name
        assert i.kernel_name.startswith(auto[1]) and (i.kernel_name == auto[1] or not auto[1].endswith(">")), i.kernel_name

    def on_lockstep(b):
        i = b.info()
        assert i.quad_path in (0, 1) and i.kernel_name.startswith("sample_kernel<"), (i.quad_path, i.kernel_name)

    def run(switch):
        b = L.LPCNetBatch(B, 0, blob)
        on_auto(b)
        out = [b.synthesize(allf[f]) for f in range(3)]
        if switch:
            b.set_kernel(1)
            on_lockstep(b)
        out += [b.synthesize(allf[f]) for f in (3, 4)]
        if switch:
            b.set_kernel(0)
            on_auto(b)
        out += list(_Frames(b, allf, 5, 9).result())
        if switch:
            b.set_kernel(1)
            on_lockstep(b)
        hf = b.host_features()
        np.copyto(hf, allf[9])
        out.append(np.array(b.synthesize_host()))
        snaps = [bytes(b.save_state(s)) for s in range(B)]
        states = [b.get_state(s) for s in range(B)]
        b.close()
        return np.stack(out, 0), snaps, states

    got, snaps, states = run(True)
    bad = np.nonzero((got != exp).any(axis=2))
    assert not len(bad[0]), ("(frame, stream)", list(zip(bad[0][:8], bad[1][:8])))
    for s in range(B):
        a, g = refs[s].state()
        assert np.array_equal(bits(states[s]["gru_a_state"]), bits(a)), s
        assert np.array_equal(bits(states[s]["gru_b_state"]), bits(g)), s
        assert states[s]["frame_count"] == refs[s].frame_count(), s
    plain, psnaps, _ = run(False)
    assert np.array_equal(plain, exp)
    assert len(snaps[0]) == STATE.itemsize
    for s in range(B):
        assert not state_diff(snaps[s], psnaps[s]), (s, state_diff(snaps[s], psnaps[s]))
        assert snaps[s] == psnaps[s], s


def _constants_fixture(name):
    G = np.load(os.path.join(O.GOLDEN, name + ".npz"))
    g, d, e = G["constants"]
    return G, (float(g), int(d), int(e))


def _replan_sequence(b, c, allf, per, wide):
    """set_model_constants, `per` frames, set_kernel(1) (re-plans a wide
    batch), `per` frames, set_kernel(0) (re-plans back), `per` frames."""
    assert b.info().quad_path == wide
    check_info_constants(b, DEFAULTS)
    b.set_model_constants(c[0], c[1], bool(c[2]))
    check_info_constants(b, c)
    out = [b.synthesize(allf[f]) for f in range(per)]
    b.set_kernel(1)
    assert b.info().quad_path in (0, 1)
    check_info_constants(b, c)
    out += [b.synthesize(allf[f]) for f in range(per, 2 * per)]
    b.set_kernel(0)
    assert b.info().quad_path == wide
    check_info_constants(b, c)
    out += [b.synthesize(allf[f]) for f in range(2 * per, 3 * per)]
    return np.stack(out, 0)


@pytest.mark.parametrize("name", ["streams_int8_g092_d3", "streams_int8_g095_d0", "streams_int8_e2e_g09_d1"])
def test_constants_survive_replan(require_gpu, monkeypatch, name):
    """lpcnet_batch_set_model_constants on a plain blob (no constant records:
    a reload from it gives 1.0 / 2 / 0), then set_kernel(1) and set_kernel(0)
    on a wide batch (8 streams, LPCNET_MFW=1: the smallest whose plan class
    is "wide"), each of which re-plans the register tables from the kept
    blob.  The constants hold "until the next load" (lpcnet_mi355x.h): the
    fixture's streams (slots 0, 1) equal the golden PCM on all nine frames,
    the other streams equal the oracle with the constants, info() reports
    them after every setter.  Guards (CPU): the frames after the first
    re-plan differ, on every stream, from the PCM of the blob's own
    constants, and from the PCM of a stream whose constants fall back to
    them at that frame."""
    for k in ("LPCNET_MFW_G", "LPCNET_MF2"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LPCNET_MFW", "1")
    G, c = _constants_fixture(name)
    B, per = 8, 3
    F = 3 * per
    blob = L.synthetic_model(1, 0)
    n = len(G["streams"])
    allf = np.stack([feats(s, F) for s in range(B)], 1)
    allf[:, :n] = G["features"][:, :F, :20].transpose(1, 0, 2)
    allf = np.ascontiguousarray(allf)
    exp, _ = expected(blob, 0, allf, constants=c)
    assert np.array_equal(exp[:, :n], G["pcm"][:, :F].transpose(1, 0, 2))
    after = np.arange(per, F)
    assert_guard(exp, expected(blob, 0, allf)[0], after, "blob constants throughout")
    assert_guard(exp, expected(blob, 0, allf, constants=c, switch=(per, DEFAULTS))[0], after, "fall back at the re-plan")
    b = L.LPCNetBatch(B, 0, blob)
    got = _replan_sequence(b, c, allf, per, 7)
    b.close()
    for s in range(n):
        assert np.array_equal(got[:, s], G["pcm"][s, :F]), ("golden", s, np.nonzero((got[:, s] != G["pcm"][s, :F]).any(1))[0])
    bad = np.nonzero((got != exp).any(axis=2))
    assert not len(bad[0]), ("(frame, stream)", list(zip(bad[0][:8], bad[1][:8])))


def test_constants_survive_replan_at_natural_width(require_gpu, monkeypatch):
    """The same on the natural trigger: 1032 streams are one mf_kernel<4>
    round of a 256-CU device plus one 8-stream workgroup, so the automatic
    kernel is mfw_kernel without any switch (quad_path 7: that assertion is
    the 256-CU assumption).  2 + 2 + 2 frames with 0.92 / 3 / 0: under these
    frame 2 is still silent, under the blob's 1.0 / 2 / 0 it is not."""
    for k in ("LPCNET_MFW", "LPCNET_MFW_G", "LPCNET_MF2"):
        monkeypatch.delenv(k, raising=False)
    c = (0.92, 3, 0)
    B, per = 1032, 2
    F = 3 * per
    check = (0, 516, 1031)
    blob = L.synthetic_model(1, 0)
    allf = np.ascontiguousarray(np.stack([feats(s, F) for s in range(B)], 1))
    sub = np.ascontiguousarray(allf[:, check])
    exp, _ = expected(blob, 0, sub, constants=c)
    after = np.arange(per, F)
    assert_guard(exp, expected(blob, 0, sub)[0], after, "blob constants throughout")
    assert_guard(exp, expected(blob, 0, sub, constants=c, switch=(per, DEFAULTS))[0], after, "fall back at the re-plan")
    b = L.LPCNetBatch(B, 0, blob)
    got = _replan_sequence(b, c, allf, per, 7)
    b.close()
    for k, s in enumerate(check):
        assert np.array_equal(got[:, s], exp[:, k]), (s, np.nonzero((got[:, s] != exp[:, k]).any(1))[0])


@pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref (the reference's compiled kernels) not built")
def test_constants_survive_rcp_table_change(require_gpu, monkeypatch):
    """set_model_constants, then set_rcp_table with this host's rcpps on a
    wide batch: on an AMD host that is a custom table, which takes the batch
    off the wide kernel and re-plans; on an Intel host the tables agree and
    nothing moves.  Either way seven frames equal the reference's kernels
    running live on this CPU with the constants, on every stream; back on
    the default table (re-plans back) and after a reset, seven frames equal
    the port oracle with the constants."""
    for k in ("LPCNET_MFW_G", "LPCNET_MF2"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LPCNET_MFW", "1")
    c = (0.92, 3, 0)
    B, F = 8, 7
    tab, bad = L.host_rcp_table()
    assert bad == 0, "this host's rcpps is not a 12-bit exponent-invariant table"
    intel = np.array_equal(tab[::2], L.rcp_table()) and np.array_equal(tab[1::2], L.rcp_table())
    blob = L.synthetic_model(1, 0)
    allf = np.ascontiguousarray(np.stack([feats(s, F) for s in range(B)], 1))
    b = L.LPCNetBatch(B, 0, blob)
    assert b.info().quad_path == 7
    b.set_model_constants(*c)
    check_info_constants(b, c)
    b.set_rcp_table(tab)
    print(f"host rcpps {'equals' if intel else 'differs from'} the Intel table: "
          f"{'no re-plan, still mfw_kernel' if intel else 're-planned for mf_kernel (table-only form)'}")
    assert b.info().quad_path == (7 if intel else 4)
    check_info_constants(b, c)
    refs = [O.Oracle(blob, 0, O.ref_kernels(), constants=c) for _ in range(B)]
    for f in range(F):
        out = b.synthesize(allf[f])
        for s in range(B):
            assert np.array_equal(out[s], refs[s].synthesize(allf[f, s])), (f, s)
    b.set_rcp_table(None)
    assert b.info().quad_path == 7
    check_info_constants(b, c)
    b.reset()
    exp, _ = expected(blob, 0, allf, constants=c)
    assert_guard(exp, expected(blob, 0, allf)[0], np.arange(2, F), "blob constants throughout")
    got = np.stack([b.synthesize(allf[f]) for f in range(F)], 0)
    b.close()
    bad = np.nonzero((got != exp).any(axis=2))
    assert not len(bad[0]), ("(frame, stream)", list(zip(bad[0][:8], bad[1][:8])))


def test_constants_change_between_frames(require_gpu):
    """Four frames at LPC_GAMMA 1.0 enqueued with an unsynchronised
    lpcnet_batch_synthesize_frames, then set_model_constants(0.9, 2, 0)
    straight away, then four more frames: the queued frames keep the
    constants they were enqueued with, the later ones take the new gamma --
    one Oracle per stream whose gamma changes at the same boundary.  Guard
    (CPU): the last four frames differ from gamma 1.0 throughout."""
    B, F = 2, 8
    blob = L.synthetic_model(1, 0)
    c = (0.9, 2, 0)
    allf = np.ascontiguousarray(np.stack([feats(s, F) for s in range(B)], 1))
    exp, refs = expected(blob, 0, allf, switch=(4, c))
    assert_guard(exp, expected(blob, 0, allf)[0], np.arange(4, F), "gamma 1.0 throughout")
    b = L.LPCNetBatch(B, 0, blob)
    queued = _Frames(b, allf, 0, 4)
    b.set_model_constants(*c)
    check_info_constants(b, c)
    got = np.concatenate([queued.result(), np.stack([b.synthesize(allf[f]) for f in range(4, F)])], 0)
    bad = np.nonzero((got != exp).any(axis=2))
    assert not len(bad[0]), ("(frame, stream)", list(zip(bad[0][:8], bad[1][:8])))
    for s in range(B):
        a, g = refs[s].state()
        st = b.get_state(s)
        assert np.array_equal(bits(st["gru_a_state"]), bits(a)) and np.array_equal(bits(st["gru_b_state"]), bits(g)), s


@pytest.mark.parametrize("B,check", [(3, (0, 1, 2)), (300, (0, 150, 299))])
def test_engine_feature_buffer_with_preload(require_gpu, B, check):
    """The batch's own feature buffer (lpcnet_batch_host_features: host-visible
    VRAM on large-BAR devices) as the source of every frame, teacher-forced
    calls included: frames 4 and 6 hand the buffer's own pointer to
    lpcnet_batch_synthesize_impl with preload 80 and 160 (the per-frame path
    with its feature copy, at 300 streams too: preload keeps a call off the
    chunked tick), the others run synthesize_host().  Against the oracle as
    test_preload_teacher_forcing_matches_oracle compares; the teacher's
    samples are echoed in the output."""
    F = 9
    blob = L.synthetic_model(1, 0)
    allf = np.stack([feats(s, F) for s in range(B)], 1)
    b = L.LPCNetBatch(B, 0, blob)
    hf = b.host_features()
    assert hf.shape == (B, 20) and hf.dtype == np.float32
    # what synthesize_impl makes of its features argument: the buffer itself, no copy
    passed = np.ascontiguousarray(np.asarray(hf, np.float32)[:, :L.NB_FEATURES])
    assert np.shares_memory(passed, hf) and passed.ctypes.data == hf.ctypes.data
    refs = {s: O.Oracle(blob, 0) for s in check}
    t = np.arange(160)
    for f in range(F):
        np.copyto(hf, allf[f])
        if f in (4, 6):
            pre = 80 if f == 4 else 160
            teacher = np.stack([(3000 * np.sin(0.05 * (s % 7 + 1) * t)).astype(np.int16) for s in range(B)])
            out = b.synthesize_impl(hf, teacher, pre)
            assert np.array_equal(out[:, :pre], teacher[:, :pre]), f
            for s in check:
                e = refs[s].synthesize(allf[f, s], 160, preload=teacher[s][:pre] if pre < 160 else teacher[s])
                if pre < 160:
                    e = np.concatenate([teacher[s][:pre], e[pre:]])
                assert np.array_equal(out[s], e), (f, s)
        else:
            out = np.array(b.synthesize_host())
            for s in check:
                assert np.array_equal(out[s], refs[s].synthesize(allf[f, s])), (f, s)
    b.close()
