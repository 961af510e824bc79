"""The PLC prediction network on the device (plc_kernel.hip,
lpcnet_batch_plc_*) against the CPU composition of compute_plc_pred
(tests/plc_ref.py; its own checks are in tests/test_plc_model.py).  Every
comparison is bit for bit, on uint32 views of the floats."""
import numpy as np
import pytest

import lpcnet_amd as L
import oracle_lib as O
import plc_ref as P

pytestmark = pytest.mark.gpu

NF = L.NB_FEATURES


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def state_bits(st: bytes):
    return np.frombuffer(st, np.uint32)


_BLOBS = {}


def model(shape: str) -> bytes:
    if shape not in _BLOBS:
        _BLOBS[shape] = L.synthetic_model(1, L.VARIANT_INT8, plc=shape == "default", plc_small=shape == "small")
    return _BLOBS[shape]


@pytest.mark.parametrize("shape", ["default", "small"])
@pytest.mark.parametrize("B", [1, 3, 16, 17])
def test_sequence_parity(require_gpu, shape, B):
    """8 consecutive calls mixing the zeros, FEC and update inputs: out of
    every stream and call and both GRU states after the last call.  B = 1, 3:
    a partial 16-stream tile; 16: a full one; 17: a second tile of one stream."""
    blob = model(shape)
    b = L.LPCNetBatch(B, 0, blob)
    assert b.plc_info() == L.plc_dims(blob)
    for c in range(P.NCALLS):
        x = P.batch_inputs(B, c)
        # the all-zero input also goes through the NULL form where every stream has it
        out = b.plc_predict(None if not x.any() else x)
        for s in range(B):
            assert np.array_equal(bits(out[s]), bits(P.sequence(blob, s)[0][c])), (c, s)
    for s in range(B):
        assert np.array_equal(state_bits(b.plc_save_state(s)), state_bits(P.sequence(blob, s)[1])), s
    b.close()


def test_null_input_and_discard(require_gpu):
    """in == NULL is the all-zero input (lpcnet_plc.c:161-162), out == NULL
    discards the prediction and still advances the state (:158)."""
    blob = model("small")
    B = 3
    b = L.LPCNetBatch(B, 0, blob)
    refs = [P.PlcRef(blob) for _ in range(B)]
    assert b.plc_predict(P.batch_inputs(B, 0), discard=True) is None
    for s in range(B):
        refs[s].predict(P.call_inputs(s)[0])
    out = b.plc_predict(None)
    for s in range(B):
        assert np.array_equal(bits(out[s]), bits(refs[s].predict(None))), s
        assert b.plc_save_state(s) == refs[s].save()
    b.close()


@pytest.mark.parametrize("shape", ["default", "small"])
def test_active_mask(require_gpu, shape):
    """active alternating per stream and per call: an inactive stream keeps its
    state and its out row; the active ones equal a CPU run that skipped the
    same calls."""
    blob = model(shape)
    B = 17
    b = L.LPCNetBatch(B, 0, blob)
    refs = [P.PlcRef(blob) for _ in range(B)]
    for c in range(P.NCALLS):
        active = np.array([(s + c) % 2 == 0 for s in range(B)])
        if c == 5:
            active[:] = False
        out = np.full((B, NF), np.float32(-77.25))
        b.plc_predict(P.batch_inputs(B, c), active=active, out=out)
        for s in range(B):
            if active[s]:
                exp = refs[s].predict(P.call_inputs(s)[c])
                assert np.array_equal(bits(out[s]), bits(exp)), (c, s)
            else:
                assert np.all(out[s] == np.float32(-77.25)), (c, s)
            assert np.array_equal(state_bits(b.plc_save_state(s)), state_bits(refs[s].save())), (c, s)
    b.close()


def test_save_restore_and_reset(require_gpu):
    """The PLC's plc_copy[] rollback: save, 2 calls, restore, 2 other calls.
    lpcnet_batch_reset_stream zeroes that stream's predictor state only,
    lpcnet_batch_reset every stream's; the synthesis snapshot keeps its size."""
    blob = model("small")
    B = 3
    b = L.LPCNetBatch(B, 0, blob)
    refs = [P.PlcRef(blob) for _ in range(B)]
    n = sum(b.plc_info()[2:])
    assert len(b.plc_save_state(0)) == 4 * n

    def step(c):
        out = b.plc_predict(P.batch_inputs(B, c))
        for s in range(B):
            assert np.array_equal(bits(out[s]), bits(refs[s].predict(P.call_inputs(s)[c]))), (c, s)

    step(0)
    step(1)
    snap = [b.plc_save_state(s) for s in range(B)]
    assert [refs[s].save() for s in range(B)] == snap
    step(2)
    step(3)
    for s in range(B):
        b.plc_restore_state(s, snap[s])
        refs[s].restore(snap[s])
    step(4)
    step(5)
    before = [b.plc_save_state(s) for s in range(B)]
    b.reset(1)
    assert b.plc_save_state(0) == before[0] and b.plc_save_state(2) == before[2]
    assert b.plc_save_state(1) == bytes(4 * n)
    refs[1].reset()
    step(6)
    b.plc_reset(2)
    assert b.plc_save_state(2) == bytes(4 * n) and b.plc_save_state(0) == refs[0].save()
    b.reset()
    assert all(b.plc_save_state(s) == bytes(4 * n) for s in range(B))
    # a state this engine cannot have produced is refused
    with pytest.raises(L.LPCNetError):
        b.plc_restore_state(0, np.full(n, 3, np.float32).tobytes())
    assert len(b.save_state(0)) == L.lib.lpcnet_batch_state_size()
    b.close()


def test_replan_keeps_the_plc_tables(require_gpu):
    """set_kernel / set_rcp_table re-plan the synthesis tables; the predictor's
    tables and states stay."""
    blob = model("small")
    B = 3
    b = L.LPCNetBatch(B, 0, blob)
    for c in range(4):
        if c == 1:
            b.set_kernel(1)
        if c == 2:
            b.set_kernel(0)
        if c == 3:
            b.set_rcp_table(None)
        out = b.plc_predict(P.batch_inputs(B, c))
        for s in range(B):
            assert np.array_equal(bits(out[s]), bits(P.sequence(blob, s)[0][c])), (c, s)
    b.close()


def test_device_resident_hand_off(require_gpu):
    """plc_predict_device writes [B][20] features into a device buffer that
    synthesize_frames reads as d_features: the PCM is the oracle's synthesis
    of the CPU-predicted features."""
    blob = model("default")
    B, F = 3, 5
    b = L.LPCNetBatch(B, 0, blob)
    d_in = b.device_alloc(B * P.PLC_IN * 4)
    d_feat = b.device_alloc(B * NF * 4)
    d_pcm = b.device_alloc(B * 160 * 2)
    orc = [O.Oracle(blob, 0) for _ in range(B)]
    b.reset_timers(1)
    nonzero = 0
    for c in range(F):
        x = P.batch_inputs(B, c)
        b.h2d(d_in, x)
        b.plc_predict_device(d_in, d_feat)
        b.synthesize_frames(None, d_feat, d_pcm, 1)
        b.sync()
        feat = np.zeros((B, NF), np.float32)
        pcm = np.zeros((B, 160), np.int16)
        b.d2h(feat, d_feat)
        b.d2h(pcm, d_pcm)
        for s in range(B):
            exp = P.sequence(blob, s)[0][c]
            assert np.array_equal(bits(feat[s]), bits(exp)), (c, s)
            assert np.array_equal(pcm[s], orc[s].synthesize(exp)), (c, s)
        nonzero += int(np.count_nonzero(pcm))
    assert nonzero > 0
    ms, launches = b.kernel_ms(2)
    assert launches == F and ms > 0 and b.kernel_frames(2) == F
    for p in (d_in, d_feat, d_pcm):
        b.device_free(p)
    b.close()


def test_blob_without_plc_records(require_gpu):
    """Every plc_* call refuses with the reason; synthesis is unaffected."""
    blob = L.synthetic_model(1, L.VARIANT_INT8)
    B = 2
    b = L.LPCNetBatch(B, 0, blob)
    calls = [b.plc_info, lambda: b.plc_predict(None), lambda: b.plc_predict_device(None, None), b.plc_reset,
             lambda: b.plc_save_state(0), lambda: b.plc_restore_state(0, bytes(4))]
    for call in calls:
        with pytest.raises(L.LPCNetError) as e:
            call()
        assert "no PLC records" in str(e.value)
    feats = np.stack([L.synthetic_features(s, 4)[:, :NF] for s in range(B)], 1)
    out = np.stack([b.synthesize(feats[f]) for f in range(4)], 1)
    for s in range(B):
        assert np.array_equal(out[s], O.synth_stream(blob, feats[:, s], 0)), s
    b.close()
    # an fp32 blob with PLC records loads and synthesises; the predictor refuses it
    b = L.LPCNetBatch(1, 0, L.synthetic_model(1, L.VARIANT_FP32, plc=True))
    with pytest.raises(L.LPCNetError) as e:
        b.plc_predict(None)
    assert "fp32" in str(e.value)
    b.close()


@pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref (the reference's compiled kernels) not built")
def test_table_form_matches_live_reference(require_gpu):
    """With this host's rcpps table the predictor runs its table form and
    equals the composition on the reference's compiled kernels, live on this
    CPU (as tests/test_gpu_samebox.py does for synthesis)."""
    tab, bad = L.host_rcp_table()
    assert bad == 0, "this host's rcpps is not a 12-bit exponent-invariant table"
    blob = model("default")
    B = 3
    b = L.LPCNetBatch(B, 0, blob)
    b.set_rcp_table(tab)
    intel = np.array_equal(tab[::2], L.rcp_table()) and np.array_equal(tab[1::2], L.rcp_table())
    assert b.info().rcp_hw == (1 if intel else 0)
    for c in range(P.NCALLS):
        out = b.plc_predict(P.batch_inputs(B, c))
        for s in range(B):
            assert np.array_equal(bits(out[s]), bits(P.sequence(blob, s, "ref")[0][c])), (c, s)
    for s in range(B):
        assert b.plc_save_state(s) == P.sequence(blob, s, "ref")[1]
    b.set_rcp_table(None)
    b.close()
