"""The feature extractor on the device (feat_kernel.hip,
lpcnet_batch_compute_features*) against the fixture
tests/golden/enc_features.npz (made by tests/enc_ref.py on the reference's
compiled kernels) and, where oracle/_ref is built, against enc_ref live.
Every comparison is bit for bit, on uint32 views of the floats."""
import os

import numpy as np
import pytest

import enc_ref as E
import lpcnet_amd as L
import oracle_lib as O

pytestmark = pytest.mark.gpu

NF, NTF, FRAME = L.NB_FEATURES, L.NB_TOTAL_FEATURES, L.FRAME_SIZE
PCM, FEATS = E.golden()  # [5, 12, 160] int16, [5, 12, 36] float32
NSIG, NFR = PCM.shape[:2]
FEATS.setflags(write=False)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def frame_pcm(B: int, f: int) -> np.ndarray:
    """[B, 160]: frame f of signal s % 5 for stream s."""
    return np.ascontiguousarray(PCM[np.arange(B) % NSIG, f])


_B1 = {}


def b1_run(sig: int) -> np.ndarray:
    """The device's features of one signal at B = 1, computed once."""
    if sig not in _B1:
        b = L.LPCNetBatch(1, 0)
        _B1[sig] = np.stack([b.compute_features(PCM[sig, f][None])[0] for f in range(NFR)])
        _B1[sig].setflags(write=False)
        b.close()
    return _B1[sig]


@pytest.mark.parametrize("as_float", [False, True])
def test_bit_equality(require_gpu, as_float):
    """B = 5 (a partial workgroup), one signal per stream, 12 single-frame
    calls: the fixture, live enc_ref, and the state that crosses frames."""
    b = L.LPCNetBatch(NSIG, 0)
    refs = [E.EncRef() for _ in range(NSIG)] if E.have_ref() else None
    for f in range(NFR):
        p = frame_pcm(NSIG, f)
        out = b.compute_features(p.astype(np.float32) if as_float else p)
        assert out.shape == (NSIG, NTF)
        for s in range(NSIG):
            assert same(out[s], FEATS[s, f]), (E.SIGNALS[s], f, np.flatnonzero(bits(out[s]) != bits(FEATS[s, f])))
            if refs:
                assert same(out[s], refs[s].frame(p[s])), (E.SIGNALS[s], f)
                assert b.features_save_state(s) == refs[s].state_bytes(), (E.SIGNALS[s], f)
    b.close()


def test_stream_independence(require_gpu):
    """B = 17 (whole workgroups and a last one with a single stream), the five signals
    cycled: stream s equals its signal alone at B = 1."""
    B = 17
    b = L.LPCNetBatch(B, 0)
    for f in range(NFR):
        out = b.compute_features(frame_pcm(B, f))
        for s in range(B):
            assert same(out[s], b1_run(s % NSIG)[f]), (s, f)
    for sig in range(NSIG):
        assert same(b1_run(sig), FEATS[sig]), E.SIGNALS[sig]
    b.close()


def test_active_mask(require_gpu):
    """Masks alternating per stream and per frame over 6 calls: a masked
    stream keeps its state and its output row; an active one sees the next
    frame of its signal, so it equals the reference advanced on its active
    frames only."""
    B = 17
    b = L.LPCNetBatch(B, 0)
    refs = [E.EncRef() for _ in range(B)] if E.have_ref() else None
    done = np.zeros(B, np.int64)  # frames each stream has consumed
    out = np.full((B, NTF), np.float32(-77.25))
    for call in range(6):
        act = ((np.arange(B) + call) % 2 == 0) | (np.arange(B) % 7 == call)
        if call == 4:
            act[:] = False  # nobody: nothing may move
        p = np.ascontiguousarray(PCM[np.arange(B) % NSIG, done])
        p[~act] = 12345  # what a masked stream is handed must not matter
        before = [b.features_save_state(s) for s in range(B)]
        prev = out.copy()
        ret = b.compute_features(p, active=act.astype(np.uint8), out=out)
        assert ret is out
        for s in range(B):
            if act[s]:
                assert same(out[s], FEATS[s % NSIG, done[s]]), (call, s)
                if refs:
                    assert same(out[s], refs[s].frame(p[s])), (call, s)
                    assert b.features_save_state(s) == refs[s].state_bytes(), (call, s)
            else:
                assert same(out[s], prev[s]), (call, s)
                assert b.features_save_state(s) == before[s], (call, s)
        done += act
    assert done.min() >= 2
    b.close()


def test_device_form(require_gpu):
    """nframes = 3 in one call equals three single calls; row = 20 equals the
    first 20 of row = 36; a mask on the device applies to every frame."""
    B, K = 5, 3
    pcm = np.ascontiguousarray(np.stack([frame_pcm(B, f) for f in range(K)]))  # [K, B, 160]
    single = L.LPCNetBatch(B, 0)
    exp = np.stack([single.compute_features(pcm[f]) for f in range(K)])
    single.close()
    assert same(exp, np.moveaxis(FEATS[:, :K], 0, 1))
    got = {}
    for row in (NTF, NF):
        b = L.LPCNetBatch(B, 0)
        d_pcm = b.device_alloc(pcm.nbytes)
        d_feat = b.device_alloc(K * B * row * 4)
        b.h2d(d_pcm, pcm)
        b.reset_timers(1)
        b.compute_features_device(d_pcm, d_feat, row, None, K)
        b.sync()
        got[row] = np.zeros((K, B, row), np.float32)
        b.d2h(got[row], d_feat)
        ms, launches = b.kernel_ms(3)
        assert launches == K and ms > 0 and b.kernel_frames(3) == K
        if row == NTF:
            # masked on the device: frames K..2K-1 for streams 0, 2, 4 only
            act = np.array([1, 0, 1, 0, 1], np.uint8)
            d_act = b.device_alloc(B)
            b.h2d(d_act, act)
            nxt = np.ascontiguousarray(np.stack([frame_pcm(B, K + f) for f in range(K)]))
            b.h2d(d_pcm, nxt)
            sentinel = np.full((K, B, row), np.float32(3.5))
            b.h2d(d_feat, sentinel)
            b.compute_features_device(d_pcm, d_feat, row, d_act, K)
            b.sync()
            m = np.zeros((K, B, row), np.float32)
            b.d2h(m, d_feat)
            for s in range(B):
                assert same(m[:, s], FEATS[s, K:2 * K] if act[s] else sentinel[:, s]), s
            b.device_free(d_act)
        with pytest.raises(L.LPCNetError) as e:
            b.compute_features_device(d_pcm, d_feat, 19, None, 1)
        assert "row" in str(e.value)
        b.device_free(d_pcm)
        b.device_free(d_feat)
        b.close()
    assert same(got[NTF], exp)
    assert same(got[NF], exp[:, :, :NF])


def test_state_save_restore_reset(require_gpu):
    """Save after frame 4, run to frame 8, restore, rerun: identical.
    features_reset(stream) equals a fresh stream and leaves the neighbours
    alone; lpcnet_batch_reset and reset(stream) reset the analysis state too."""
    B = 5
    b = L.LPCNetBatch(B, 0)
    with pytest.raises(L.LPCNetError):
        b.features_reset(B)
    for f in range(4):
        b.compute_features(frame_pcm(B, f))
    snap = [b.features_save_state(s) for s in range(B)]
    first = [b.compute_features(frame_pcm(B, f)) for f in range(4, 8)]
    for s in range(B):
        b.features_restore_state(s, snap[s])
    again = [b.compute_features(frame_pcm(B, f)) for f in range(4, 8)]
    assert same(np.stack(first), np.stack(again))
    assert same(np.stack(first), np.moveaxis(FEATS[:, 4:8], 0, 1))
    # back to the end of frame 3; a snapshot moves to another stream: stream 0 continues signal 3
    for s in range(B):
        b.features_restore_state(s, snap[3 if s == 0 else s])
    p = frame_pcm(B, 4)
    p[0] = PCM[3, 4]
    assert same(b.compute_features(p)[0], FEATS[3, 4])
    with pytest.raises(L.LPCNetError) as e:
        bad = bytearray(snap[0])
        bad[-4:] = (224).to_bytes(4, "little")
        b.features_restore_state(0, bytes(bad))
    assert "best_i" in str(e.value)
    # reset of stream 1: it starts over, the others go on from frame 5
    b.features_reset(1)
    p = frame_pcm(B, 5)
    p[1] = PCM[1, 0]
    out = b.compute_features(p)
    assert same(out[1], FEATS[1, 0])
    for s in (2, 3, 4):
        assert same(out[s], FEATS[s, 5]), s
    # reset_stream resets the analysis state with the synthesis state
    b.reset(2)
    p = frame_pcm(B, 6)
    p[2] = PCM[2 % NSIG, 0]
    p[1] = PCM[1, 1]
    out = b.compute_features(p)
    assert same(out[2], FEATS[2, 0]) and same(out[1], FEATS[1, 1]) and same(out[4], FEATS[4, 6])
    fresh = bytes(len(snap[0]))
    b.features_reset(None)
    assert all(b.features_save_state(s) == fresh for s in range(B))
    b.compute_features(frame_pcm(B, 0))
    assert b.features_save_state(0) != fresh
    b.reset()
    assert all(b.features_save_state(s) == fresh for s in range(B))
    assert same(b.compute_features(frame_pcm(B, 0)), FEATS[:, 0])
    b.close()


def test_no_model_and_model_changes(require_gpu):
    """The analysis has no weights: a batch without a blob, a batch with one,
    and one whose model, kernel and rcpps table change between frames all
    give the fixture."""
    B = 5
    blob = L.synthetic_model(1, L.VARIANT_INT8)
    plain = L.LPCNetBatch(B, 0)
    with pytest.raises(L.LPCNetError):
        plain.info()  # no model
    loaded = L.LPCNetBatch(B, 0, blob)
    moving = L.LPCNetBatch(B, 0)
    table, _ = L.host_rcp_table()
    for f in range(6):
        if f == 2:
            moving.load_model(blob)
            moving.set_kernel(1)
            moving.set_rcp_table(table)
        if f == 4:
            moving.load_model(L.synthetic_model(2, L.VARIANT_FP32))
            moving.set_model_constants(0.9, 1, False)
        p = frame_pcm(B, f)
        outs = [x.compute_features(p) for x in (plain, loaded, moving)]
        for o in outs:
            assert same(o, FEATS[:, f]), f
    for x in (plain, loaded, moving):
        x.close()


def test_chain_stays_on_the_device(require_gpu):
    """3 streams x 4 frames: features computed from a device PCM buffer with
    row = 20 are read by pointer by synthesize_frames (as d_features) and by
    plc_predict_device, with no synchronisation in between; the results equal
    the same calls fed the same features through host copies.  The predictor
    reads its [B][57] rows from the head of the feature buffer: the hand-off
    by pointer is what is checked here (placing a feature row at columns
    36..55 of a predictor row belongs with the Burg analysis that fills
    columns 0..35)."""
    B, K = 3, 4
    sig = [0, 1, 3]
    blob = L.synthetic_model(1, L.VARIANT_INT8, plc=True)
    pcm_in = np.ascontiguousarray(np.moveaxis(PCM[sig, :K], 0, 1))  # [K, B, 160]
    res = {}
    feat = None
    for way in ("device", "host"):
        b = L.LPCNetBatch(B, 0, blob)
        d_feat = b.device_alloc(K * B * NF * 4)
        d_pcm = b.device_alloc(K * B * FRAME * 2)
        d_plc = b.device_alloc(B * NF * 4)
        if way == "device":
            d_in = b.device_alloc(pcm_in.nbytes)
            b.h2d(d_in, pcm_in)
            b.compute_features_device(d_in, d_feat, NF, None, K)
        else:
            b.h2d(d_feat, feat)
        b.synthesize_frames(None, d_feat, d_pcm, K)
        b.plc_predict_device(d_feat, d_plc)
        b.sync()
        if way == "device":
            feat = np.zeros((K, B, NF), np.float32)
            b.d2h(feat, d_feat)
            for k, s in enumerate(sig):
                assert same(feat[:, k], FEATS[s, :K, :NF]), s
            b.device_free(d_in)
        pcm = np.zeros((K, B, FRAME), np.int16)
        plc = np.zeros((B, NF), np.float32)
        b.d2h(pcm, d_pcm)
        b.d2h(plc, d_plc)
        res[way] = (pcm, plc, [b.save_state(s) for s in range(B)], [b.plc_save_state(s) for s in range(B)])
        for p in (d_feat, d_pcm, d_plc):
            b.device_free(p)
        b.close()
    assert np.array_equal(res["device"][0], res["host"][0]) and np.count_nonzero(res["host"][0]) > 0
    assert same(res["device"][1], res["host"][1]) and np.isfinite(res["host"][1]).all()
    assert res["device"][2] == res["host"][2] and res["device"][3] == res["host"][3]
    # and the synthesis is the oracle's of those features
    for k in range(B):
        assert np.array_equal(res["device"][0][:, k], O.synth_stream(blob, feat[:, k], 0)), k


def test_existing_results_unchanged(require_gpu):
    """lpc_kernel shares its stages with feat_kernel (lpc_stages.h): device_lpc
    and the synthesis golden, 3 streams x 6 frames, on a batch that also
    extracts features."""
    K = np.load(os.path.join(O.GOLDEN, "kernels.npz"))
    ceps = np.ascontiguousarray(K["lpc_ceps"], np.float32)[:, :18]
    assert np.array_equal(L.device_lpc(ceps).view(np.uint32), np.asarray(K["lpc_out"], np.float32).view(np.uint32))
    G = np.load(os.path.join(O.GOLDEN, "streams_int8.npz"))
    B = 3
    b = L.LPCNetBatch(B, 0, L.synthetic_model(1, L.VARIANT_INT8))
    for fr in range(6):
        assert same(b.compute_features(frame_pcm(B, fr)), FEATS[:B, fr])
        assert np.array_equal(b.synthesize(G["features"][:B, fr, :NF]), G["pcm"][:B, fr]), fr
    b.close()
