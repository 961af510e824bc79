"""The DRED RDO-VAE on the device (rdovae_kernel.hip, lpcnet_batch_rdovae_*)
against the CPU composition of dred_rdovae_encode_dframe, dec_init_states,
decode_qframe and DRED_rdovae_decode_all (tests/rdovae_ref.py; its own checks
are in tests/test_rdovae_model.py).  Every comparison is bit for bit, on
uint32 views of the floats."""
import os

import numpy as np
import pytest

import lpcnet_amd as L
import oracle_lib as O
import rdovae_ref as R

pytestmark = pytest.mark.gpu

NF = L.NB_FEATURES
FILL = np.float32(-77.25)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def state_bits(st: bytes):
    return np.frombuffer(st, np.uint32)


_BLOBS = {}


def model(shape: str) -> bytes:
    if shape not in _BLOBS:
        _BLOBS[shape] = L.synthetic_model(1, L.VARIANT_INT8, rdovae=shape == "default", rdovae_small=shape == "small")
    return _BLOBS[shape]


def dec_inputs(blob, B, n=R.NDEC):
    d = L.rdovae_dims(blob)["dec"]
    st = np.stack([R.dec_state(s, d["S"]) for s in range(B)])
    z = np.stack([R.dec_latents(s, d["L"])[:n] for s in range(B)])
    return st, z


@pytest.mark.parametrize("shape", ["default", "small"])
@pytest.mark.parametrize("B", [1, 3, 16, 17])
def test_encoder_sequence_parity(require_gpu, shape, B):
    """6 consecutive calls (the 4-tap conv memory has wrapped completely):
    latents and initial state of every call and stream, and the saved state
    after the last.  B = 1, 3: a partial 16-stream tile; 16: a full one; 17: a
    second tile of one stream."""
    blob = model(shape)
    b = L.LPCNetBatch(B, 0, blob)
    assert b.rdovae_info() == L.rdovae_dims(blob)
    for c in range(R.NENC):
        z, st = b.rdovae_encode(R.enc_batch(B, c))
        for s in range(B):
            ref = R.enc_sequence(blob, s)
            assert np.array_equal(bits(z[s]), bits(ref[0][c])), (c, s)
            assert np.array_equal(bits(st[s]), bits(ref[1][c])), (c, s)
    for s in range(B):
        assert np.array_equal(state_bits(b.rdovae_save_state(s, 1)), state_bits(R.enc_sequence(blob, s)[2])), s
    b.close()


@pytest.mark.parametrize("shape", ["default", "small"])
@pytest.mark.parametrize("B", [1, 3, 16, 17])
def test_decoder_parity(require_gpu, shape, B):
    """dec_init, then 4 qframes: every qframe and the final states."""
    blob = model(shape)
    b = L.LPCNetBatch(B, 0, blob)
    st, z = dec_inputs(blob, B)
    b.rdovae_dec_init(st)
    for c in range(R.NDEC):
        q = b.rdovae_decode_qframe(z[:, c])
        for s in range(B):
            assert np.array_equal(bits(q[s]), bits(R.dec_sequence(blob, s)[0][c])), (c, s)
    for s in range(B):
        assert np.array_equal(state_bits(b.rdovae_save_state(s, 2)), state_bits(R.dec_sequence(blob, s)[1])), s
    b.close()


@pytest.mark.parametrize("shape", ["default", "small"])
@pytest.mark.parametrize("n", [1, 3])
def test_decode_all_parity(require_gpu, shape, n):
    """decode_all equals the reference, equals dec_init + n qframes on a
    fresh batch, and leaves a previously set persistent decoder state
    bit-unchanged."""
    blob = model(shape)
    B = 17
    b = L.LPCNetBatch(B, 0, blob)
    st, z = dec_inputs(blob, B, n)
    # a persistent state that is not the reset one
    b.rdovae_dec_init(st[::-1])
    b.rdovae_decode_qframe(z[::-1, 0])
    before = [b.rdovae_save_state(s, 2) for s in range(B)]
    assert any(before[s] != bytes(len(before[s])) for s in range(B))
    f = b.rdovae_decode_all(st, z)
    assert f.shape == (B, 4 * n, NF)
    for s in range(B):
        assert np.array_equal(bits(f[s]), bits(R.all_sequence(blob, s, n))), s
    assert [b.rdovae_save_state(s, 2) for s in range(B)] == before
    # n == 0 is a no-op
    assert b.rdovae_decode_all(st, z[:, :0]).shape == (B, 0, NF)
    b.close()
    b = L.LPCNetBatch(B, 0, blob)
    b.rdovae_dec_init(st)
    q = np.stack([b.rdovae_decode_qframe(z[:, c]) for c in range(n)], 1)  # [B, n, 80]
    assert np.array_equal(bits(q.reshape(B, 4 * n, NF)), bits(f))
    b.close()


def test_active_mask_encoder(require_gpu):
    """active alternating per stream and per call: an inactive stream keeps
    its state and its output rows; the active ones equal a CPU run that
    skipped the same calls."""
    blob = model("small")
    B = 17
    b = L.LPCNetBatch(B, 0, blob)
    refs = [R.RdoEnc(blob) for _ in range(B)]
    d = L.rdovae_dims(blob)["enc"]
    for c in range(4):
        active = np.array([(s + c) % 2 == 0 for s in range(B)])
        if c == 2:
            active[:] = False
        z = np.full((B, d["L"]), FILL)
        st = np.full((B, d["S"]), FILL)
        b.rdovae_encode(R.enc_batch(B, c), active=active, latents=z, state=st)
        for s in range(B):
            if active[s]:
                ez, est = refs[s].encode(R.enc_inputs(s)[c])
                assert np.array_equal(bits(z[s]), bits(ez)) and np.array_equal(bits(st[s]), bits(est)), (c, s)
            else:
                assert np.all(z[s] == FILL) and np.all(st[s] == FILL), (c, s)
            assert np.array_equal(state_bits(b.rdovae_save_state(s, 1)), state_bits(refs[s].save())), (c, s)
    b.close()


def test_active_mask_decoder(require_gpu):
    blob = model("small")
    B = 17
    b = L.LPCNetBatch(B, 0, blob)
    refs = [R.RdoDec(blob) for _ in range(B)]
    st, z = dec_inputs(blob, B)
    init_active = np.array([s % 3 != 1 for s in range(B)])
    b.rdovae_dec_init(st, active=init_active)
    for s in range(B):
        if init_active[s]:
            refs[s].init(st[s])
        assert np.array_equal(state_bits(b.rdovae_save_state(s, 2)), state_bits(refs[s].save())), s
    for c in range(3):
        active = np.array([(s + c) % 2 == 0 for s in range(B)])
        q = np.full((B, 4 * NF), FILL)
        b.rdovae_decode_qframe(z[:, c], active=active, out=q)
        for s in range(B):
            if active[s]:
                assert np.array_equal(bits(q[s]), bits(refs[s].qframe(z[s, c]))), (c, s)
            else:
                assert np.all(q[s] == FILL), (c, s)
            assert np.array_equal(state_bits(b.rdovae_save_state(s, 2)), state_bits(refs[s].save())), (c, s)
    # decode_all: inactive rows untouched
    active = np.array([s % 2 == 1 for s in range(B)])
    f = np.full((B, 8, NF), FILL)
    b.rdovae_decode_all(st, z[:, :2], active=active, out=f)
    for s in range(B):
        if active[s]:
            assert np.array_equal(bits(f[s]), bits(R.decode_all(blob, st[s], z[s, :2]))), s
        else:
            assert np.all(f[s] == FILL), s
    b.close()


def test_state_handling(require_gpu):
    """reset with which = 1 / 2 / 3; save, diverge, restore, continue; a state
    of the wrong size is refused; the other snapshot sizes are unchanged."""
    blob = L.synthetic_model(1, L.VARIANT_INT8, plc_small=True, rdovae_small=True)
    B = 3
    b = L.LPCNetBatch(B, 0, blob)
    sizes = (L.lib.lpcnet_batch_state_size(), L.lib.lpcnet_batch_features_state_size(b._b),
             L.lib.lpcnet_batch_encode_state_size(b._b), L.lib.lpcnet_batch_plc_state_size(b._b))
    assert sizes[3] == 4 * sum(L.plc_dims(blob)[2:])
    d = L.rdovae_dims(blob)
    ne = (sum(d["enc"]["widths"][1:6:2]) + (d["enc"]["kernel"] - 1) * d["enc"]["T"]) * 4
    nd = sum(d["dec"]["widths"][1:6:2]) * 4
    assert len(b.rdovae_save_state(0, 1)) == ne and len(b.rdovae_save_state(0, 2)) == nd
    assert len(b.rdovae_save_state(0)) == ne + nd
    enc = [R.RdoEnc(blob) for _ in range(B)]

    def step(c):
        z, st = b.rdovae_encode(R.enc_batch(B, c))
        for s in range(B):
            ez, est = enc[s].encode(R.enc_inputs(s)[c])
            assert np.array_equal(bits(z[s]), bits(ez)) and np.array_equal(bits(st[s]), bits(est)), (c, s)

    step(0)
    step(1)
    snap = [b.rdovae_save_state(s, 1) for s in range(B)]
    assert snap == [e.save() for e in enc]
    step(2)
    step(3)
    # restore and continue with other inputs
    for s in range(B):
        b.rdovae_restore_state(s, snap[s], 1)
        enc[s] = R.RdoEnc(blob)
        enc[s].encode(R.enc_inputs(s)[0])
        enc[s].encode(R.enc_inputs(s)[1])
    step(4)
    st, z = dec_inputs(blob, B)
    b.rdovae_dec_init(st)
    b.rdovae_decode_qframe(z[:, 0])
    both = [b.rdovae_save_state(s) for s in range(B)]
    assert all(both[s][:ne] == enc[s].save() for s in range(B))
    # which = 2: the decoder's only, of one stream
    b.rdovae_reset(1, 2)
    assert b.rdovae_save_state(1) == both[1][:ne] + bytes(nd) and b.rdovae_save_state(0) == both[0]
    # which = 1: the encoder's only, of every stream
    b.rdovae_reset(None, 1)
    assert b.rdovae_save_state(0) == bytes(ne) + both[0][ne:] and b.rdovae_save_state(1) == bytes(ne + nd)
    # a restored whole snapshot continues both sides
    b.rdovae_restore_state(2, both[2])
    assert b.rdovae_save_state(2) == both[2]
    b.rdovae_reset(None, 3)
    assert all(b.rdovae_save_state(s) == bytes(ne + nd) for s in range(B))
    # lpcnet_batch_reset knows nothing of DRED
    b.rdovae_restore_state(0, both[0])
    b.reset()
    assert b.rdovae_save_state(0) == both[0]
    with pytest.raises(L.LPCNetError):
        b.rdovae_restore_state(0, both[0][:-4])
    with pytest.raises(L.LPCNetError):
        b.rdovae_restore_state(0, both[0], 1)
    with pytest.raises(L.LPCNetError):
        b.rdovae_restore_state(0, np.full(ne // 4, 3, np.float32).tobytes(), 1)
    with pytest.raises(L.LPCNetError):
        b.rdovae_reset(0, 4)
    assert sizes == (L.lib.lpcnet_batch_state_size(), L.lib.lpcnet_batch_features_state_size(b._b),
                     L.lib.lpcnet_batch_encode_state_size(b._b), L.lib.lpcnet_batch_plc_state_size(b._b))
    assert len(b.save_state(0)) == sizes[0] and len(b.features_save_state(0)) == sizes[1]
    b.close()


@pytest.mark.parametrize("row", [20, 36])
def test_device_resident_hand_off(require_gpu, row):
    """compute_features_device (2 frames) -> rdovae_encode_device ->
    rdovae_decode_all_device (n = 1), against the same chain through host
    arrays; the launches are timed as regions 8 and 9."""
    blob = model("small")
    B = 5
    d = L.rdovae_dims(blob)
    Ld, S = d["enc"]["L"], d["enc"]["S"]
    assert (Ld, S) == (d["dec"]["L"], d["dec"]["S"])
    rng = np.random.RandomState(31)
    pcm = (2000 * rng.randn(2, B, 160)).astype(np.int16)
    b = L.LPCNetBatch(B, 0, blob)
    d_pcm = b.device_alloc(pcm.nbytes)
    d_feat = b.device_alloc(2 * B * row * 4)
    d_lat = b.device_alloc(B * Ld * 4)
    d_st = b.device_alloc(B * S * 4)
    d_out = b.device_alloc(B * 4 * NF * 4)
    b.reset_timers(1)
    b.h2d(d_pcm, pcm)
    b.compute_features_device(d_pcm, d_feat, row, nframes=2)
    b.rdovae_encode_device(d_feat, d_lat, d_st, row)
    b.rdovae_decode_all_device(d_st, d_lat, d_out, 1)
    b.sync()
    z, st, f = np.zeros((B, Ld), np.float32), np.zeros((B, S), np.float32), np.zeros((B, 4, NF), np.float32)
    b.d2h(z, d_lat)
    b.d2h(st, d_st)
    b.d2h(f, d_out)
    assert b.kernel_ms(8)[1] == 1 and b.kernel_ms(9)[1] == 1 and b.kernel_frames(9) == 1
    assert b.kernel_ms(8)[0] > 0 and b.kernel_ms(9)[0] > 0
    for p in (d_pcm, d_feat, d_lat, d_st, d_out):
        b.device_free(p)
    b.close()
    h = L.LPCNetBatch(B, 0, blob)
    feats = np.stack([h.compute_features(pcm[k]) for k in range(2)])  # [2, B, 36]
    hz, hst = h.rdovae_encode(np.concatenate([feats[0][:, :NF], feats[1][:, :NF]], 1))
    hf = h.rdovae_decode_all(hst, hz[:, None, :])
    h.close()
    assert np.array_equal(bits(z), bits(hz)) and np.array_equal(bits(st), bits(hst)) and np.array_equal(bits(f), bits(hf))
    assert np.abs(z).max() > 1e-3


def test_blob_without_rdovae_records(require_gpu):
    """Every RDO-VAE call refuses with the reason; synthesis still matches
    the golden fixture's oracle."""
    blob = L.synthetic_model(1, L.VARIANT_INT8)
    G = np.load(os.path.join(O.GOLDEN, "streams_int8.npz"))
    B = len(G["streams"])
    b = L.LPCNetBatch(B, 0, blob)
    x = np.zeros((B, 40), np.float32)
    calls = [b.rdovae_info, lambda: b.rdovae_encode(x), lambda: b.rdovae_encode_device(None, None, None),
             lambda: b.rdovae_dec_init(x), lambda: b.rdovae_dec_init_device(None),
             lambda: b.rdovae_decode_qframe(x), lambda: b.rdovae_decode_qframe_device(None, None),
             lambda: b.rdovae_decode_all(x, x[:, None]), lambda: b.rdovae_decode_all_device(None, None, None, 1),
             b.rdovae_reset, lambda: b.rdovae_save_state(0), lambda: b.rdovae_restore_state(0, bytes(4))]
    for k, call in enumerate(calls):
        with pytest.raises(L.LPCNetError) as e:
            call()
        assert "carries no" in str(e.value), k
    for fr in range(4):
        assert np.array_equal(b.synthesize(G["features"][:, fr, :NF]), G["pcm"][:, fr]), fr
    b.close()
    # an fp32 blob with the records loads and synthesises; the RDO-VAE refuses it
    b = L.LPCNetBatch(1, 0, L.synthetic_model(1, L.VARIANT_FP32, rdovae_small=True))
    with pytest.raises(L.LPCNetError) as e:
        b.rdovae_encode(np.zeros((1, 40), np.float32))
    assert "fp32" in str(e.value)
    b.close()


def test_replan_keeps_the_rdovae_tables(require_gpu):
    """set_kernel / set_rcp_table re-plan the synthesis tables; the RDO-VAE's
    tables and states stay."""
    blob = model("small")
    B = 3
    b = L.LPCNetBatch(B, 0, blob)
    st, z = dec_inputs(blob, B)
    b.rdovae_dec_init(st)
    for c in range(4):
        if c == 1:
            b.set_kernel(1)
        if c == 2:
            b.set_kernel(0)
        if c == 3:
            b.set_rcp_table(None)
        zz, ss = b.rdovae_encode(R.enc_batch(B, c))
        q = b.rdovae_decode_qframe(z[:, c])
        for s in range(B):
            assert np.array_equal(bits(zz[s]), bits(R.enc_sequence(blob, s)[0][c])), (c, s)
            assert np.array_equal(bits(ss[s]), bits(R.enc_sequence(blob, s)[1][c])), (c, s)
            assert np.array_equal(bits(q[s]), bits(R.dec_sequence(blob, s)[0][c])), (c, s)
    b.close()


@pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref (the reference's compiled kernels) not built")
def test_table_form_matches_live_reference(require_gpu):
    """With this host's rcpps table the kernel runs its table form and equals
    the composition on the reference's compiled kernels, live on this CPU."""
    tab, bad = L.host_rcp_table()
    assert bad == 0, "this host's rcpps is not a 12-bit exponent-invariant table"
    blob = model("default")
    B = 3
    b = L.LPCNetBatch(B, 0, blob)
    b.set_rcp_table(tab)
    st, z = dec_inputs(blob, B)
    b.rdovae_dec_init(st)
    for c in range(R.NDEC):
        zz, ss = b.rdovae_encode(R.enc_batch(B, c))
        q = b.rdovae_decode_qframe(z[:, c])
        for s in range(B):
            assert np.array_equal(bits(zz[s]), bits(R.enc_sequence(blob, s, "ref")[0][c])), (c, s)
            assert np.array_equal(bits(ss[s]), bits(R.enc_sequence(blob, s, "ref")[1][c])), (c, s)
            assert np.array_equal(bits(q[s]), bits(R.dec_sequence(blob, s, "ref")[0][c])), (c, s)
    for s in range(B):
        assert b.rdovae_save_state(s, 2) == R.dec_sequence(blob, s, "ref")[1]
    b.set_rcp_table(None)
    b.close()


def test_one_sided_blobs(require_gpu):
    """An encoder-only and a decoder-only blob are each accepted for their
    side; the other side's calls refuse with the reason."""
    from test_rdovae_model import DEC_NAMES, ENC_NAMES, strip
    blob = model("small")
    B = 3
    st, z = dec_inputs(blob, B)
    b = L.LPCNetBatch(B, 0, strip(blob, set(DEC_NAMES)))
    assert b.rdovae_info()["dec"] is None
    zz, ss = b.rdovae_encode(R.enc_batch(B, 0))
    for s in range(B):
        assert np.array_equal(bits(zz[s]), bits(R.enc_sequence(blob, s)[0][0])), s
        assert np.array_equal(bits(ss[s]), bits(R.enc_sequence(blob, s)[1][0])), s
    for call in (lambda: b.rdovae_dec_init(st), lambda: b.rdovae_save_state(0), lambda: b.rdovae_reset(None, 2)):
        with pytest.raises(L.LPCNetError) as e:
            call()
        assert "carries no dec_dense1..8 records" in str(e.value)
    b.rdovae_reset(None, 1)
    assert b.rdovae_save_state(0, 1) == bytes(len(b.rdovae_save_state(0, 1)))
    b.close()
    b = L.LPCNetBatch(B, 0, strip(blob, set(ENC_NAMES)))
    assert b.rdovae_info()["enc"] is None
    b.rdovae_dec_init(st)
    q = b.rdovae_decode_qframe(z[:, 0])
    for s in range(B):
        assert np.array_equal(bits(q[s]), bits(R.dec_sequence(blob, s)[0][0])), s
    with pytest.raises(L.LPCNetError) as e:
        b.rdovae_encode(R.enc_batch(B, 0))
    assert "carries no enc_dense1..8 records" in str(e.value)
    b.close()
