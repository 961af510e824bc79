"""The 1.6 kb/s encoder on the device (feat_kernel.hip's superframe form,
enc_kernel.hip; lpcnet_batch_encode*, lpcnet_batch_compute_features4) against
the committed fixture tests/golden/enc_packets.npz, which
tests/enc_packet_ref.py made on the reference's compiled kernels.  Every
comparison is bit for bit: packets as bytes, floats as uint32 views."""
import importlib.util
import os

import numpy as np
import pytest

import enc_packet_ref as P
import feat_signals as FS
import lpcnet_amd as L
import oracle_lib as O

pytestmark = pytest.mark.gpu

NF, NTF, FRAME = L.NB_FEATURES, L.NB_TOTAL_FEATURES, L.FRAME_SIZE
FX = P.fixture()
S, NP = FX["pcm"].shape[0], P.NPACKETS
PCM = FX["pcm"].reshape(S, NP, 4 * FRAME)  # [24, 6, 640]
BLOB = L.synthetic_model(1, L.VARIANT_INT8, codebooks=True)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def pcm_of(B: int, p: int) -> np.ndarray:
    """[B, 640]: packet p of signal s % 24 for stream s."""
    return np.ascontiguousarray(PCM[np.arange(B) % S, p])


_RUN = {}


def run_all():
    """B = 24, one signal per stream, six lpcnet_batch_encode calls, computed
    once: (packets [6, 24, 8], features [6, 4, 24, 36], states [24])."""
    if not _RUN:
        b = L.LPCNetBatch(S, 0, BLOB)
        pk, ft = [], []
        for p in range(NP):
            a, f = b.encode(pcm_of(S, p))
            pk.append(a)
            ft.append(f)
        _RUN["v"] = (np.stack(pk), np.stack(ft), [b.encode_save_state(s) for s in range(S)])
        for v in _RUN["v"][:2]:
            v.setflags(write=False)
        b.close()
    return _RUN["v"]


@pytest.mark.parametrize("B", [24, 23])
def test_bit_equality(require_gpu, B):
    """Packets, quantised features, unquantised features and the state after
    the last packet; B = 23 leaves the last workgroups ragged."""
    if B == S:
        pk, ft, st = run_all()
    else:
        b = L.LPCNetBatch(B, 0, BLOB)
        r = [b.encode(pcm_of(B, p)) for p in range(NP)]
        pk, ft = np.stack([x[0] for x in r]), np.stack([x[1] for x in r])
        st = [b.encode_save_state(s) for s in range(B)]
        b.close()
    for s in range(B):
        for p in range(NP):
            assert bytes(pk[p, s]) == bytes(FX["packets"][s, p]), (FX["names"][s], p, P.unpack(pk[p, s]), P.unpack(FX["packets"][s, p]))
            assert same(ft[p, :, s], FX["qfeat"][s, p]), (FX["names"][s], p, np.argwhere(bits(ft[p, :, s]) != bits(FX["qfeat"][s, p])).tolist())
        assert st[s] == FX["state_enc"][s].tobytes(), (FX["names"][s], FS.state_diff(st[s][:FS.STATE_SIZE], FX["state_enc"][s].tobytes()[:FS.STATE_SIZE]))
    b = L.LPCNetBatch(B, 0)  # lpcnet_compute_features needs no model
    for p in range(NP):
        f = b.compute_features4(pcm_of(B, p))
        for s in range(B):
            assert same(f[:, s], FX["ufeat"][s, p]), (FX["names"][s], p, np.argwhere(bits(f[:, s]) != bits(FX["ufeat"][s, p])).tolist())
    for s in range(B):
        assert b.encode_save_state(s) == FX["state_feat"][s].tobytes(), FX["names"][s]
    assert len(b.features_save_state(0)) == FS.STATE_SIZE
    assert b.encode_save_state(0)[:FS.STATE_SIZE] == b.features_save_state(0)
    b.close()


def test_ties(require_gpu):
    """Codebooks whose rows repeat (entry i + 512 = entry i per stage, i + 2048
    = i in the difference codebook, an all-zero row pair): every minimum has an
    equal partner later in the serial order, which must lose."""
    spec = importlib.util.spec_from_file_location("append_codebooks", os.path.join(O.ROOT, "tools", "append_codebooks.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    cb = P.tie_codebooks(P.fixture_codebooks())
    flat = np.concatenate([cb[n] for n, _ in tool.SHAPES])
    blob = tool.append_codebooks(BLOB, flat)
    assert P.blob_codebooks(blob)["ceps_codebook2"].reshape(1024, 17)[519].any() == 0
    b = L.LPCNetBatch(S, 0, blob)
    for p in range(NP):
        pk, _ = b.encode(pcm_of(S, p), want_features=False)
        for s in range(S):
            assert bytes(pk[s]) == bytes(FX["tie_packets"][s, p]), (FX["names"][s], p, P.unpack(pk[s]), P.unpack(FX["tie_packets"][s, p]))
    b.close()


def test_stream_independence(require_gpu):
    """Stream s of the batch of 24 equals its signal alone at B = 1."""
    pk, ft, st = run_all()
    for s in (0, 7, 16, 20, 23):
        b = L.LPCNetBatch(1, 0, BLOB)
        for p in range(NP):
            a, f = b.encode(PCM[s, p][None])
            assert bytes(a[0]) == bytes(pk[p, s]) and same(f[:, 0], ft[p, :, s]), (s, p)
        assert b.encode_save_state(0) == st[s], s
        b.close()


def test_active_mask(require_gpu):
    """Every third stream sits out packet 1's call: its packet, feature rows
    and state are untouched, and its later results are as if the call had not
    happened (it sees packet 1 one call later)."""
    pk, ft, st = run_all()
    b = L.LPCNetBatch(S, 0, BLOB)
    act = (np.arange(S) % 3 != 0).astype(np.uint8)
    done = np.zeros(S, np.int64)
    for call in range(NP):
        masked = call == 1
        x = np.ascontiguousarray(PCM[np.arange(S), done])
        opk = np.full((S, 8), 0xA5, np.uint8)
        oft = np.full((4, S, NTF), np.float32(-77.25))
        if masked:
            x[act == 0] = 12345  # what a masked stream is handed must not matter
            before = [b.encode_save_state(s) for s in range(S)]
        b.encode(x, active=act if masked else None, packets=opk, features=oft)
        for s in range(S):
            if masked and not act[s]:
                assert (opk[s] == 0xA5).all() and (oft[:, s] == np.float32(-77.25)).all(), s
                assert b.encode_save_state(s) == before[s], s
            else:
                assert bytes(opk[s]) == bytes(pk[done[s], s]) and same(oft[:, s], ft[done[s], :, s]), (call, s)
        done += 1 if not masked else act
    b.close()


def test_one_state(require_gpu):
    """Single-frame extraction and lpcnet_encode alternate on the same streams:
    one LPCNetEncState (the Viterbi rows are shared)."""
    b = L.LPCNetBatch(S, 0, BLOB)
    for k in range(NP // 2):
        x = pcm_of(S, 2 * k).reshape(S, 4, FRAME)
        for fr in range(4):
            f = b.compute_features(np.ascontiguousarray(x[:, fr]))
            for s in range(S):
                assert same(f[s], FX["mix_single"][s, k, fr]), (FX["names"][s], k, fr)
        pk, ft = b.encode(pcm_of(S, 2 * k + 1))
        for s in range(S):
            assert bytes(pk[s]) == bytes(FX["mix_packets"][s, k]), (FX["names"][s], k)
            assert same(ft[:, s], FX["mix_qfeat"][s, k]), (FX["names"][s], k)
    for s in range(S):
        assert b.encode_save_state(s) == FX["mix_state"][s].tobytes(), FX["names"][s]
    b.close()


def test_state_snapshots_and_reset(require_gpu):
    pk, ft, st = run_all()
    b = L.LPCNetBatch(S, 0, BLOB)
    for p in range(3):
        b.encode(pcm_of(S, p), want_features=False)
    snap = [b.encode_save_state(s) for s in range(S)]
    assert len(snap[0]) == FS.STATE_SIZE + 4 * P.NB and len(b.features_save_state(0)) == FS.STATE_SIZE
    for p in range(3, NP):
        b.encode(pcm_of(S, p), want_features=False)
    for s in range(S):
        b.encode_restore_state(s, snap[s])
    for p in range(3, NP):
        a, f = b.encode(pcm_of(S, p))
        assert a.tobytes() == pk[p].tobytes() and same(f, ft[p]), p
    # one stream back to packet 0; the others go on from their state
    b.reset(5)
    a, f = b.encode(pcm_of(S, 0))
    assert bytes(a[5]) == bytes(pk[0, 5]) and same(f[:, 5], ft[0, :, 5])
    b.features_reset(6)
    a, f = b.encode(pcm_of(S, 0))
    assert bytes(a[6]) == bytes(pk[0, 6]) and same(f[:, 6], ft[0, :, 6])
    b.reset()
    a, f = b.encode(pcm_of(S, 0))
    assert a.tobytes() == pk[0].tobytes() and same(f, ft[0])
    with pytest.raises(L.LPCNetError):
        b.encode_restore_state(0, snap[0][:-4])
    b.close()


@pytest.mark.parametrize("row", [NF, NTF])
def test_device_form(require_gpu, row):
    """encode_device with npackets = 6 equals six host calls, for both row
    widths; the packets then feed lpcnet_batch_decode_frames on a second batch
    without leaving device memory, whose PCM equals synthesising the encoder's
    own features: both batches hold the same 20 decoded values per frame.
    (Streams whose packets carry less than the encoder's features use -- a
    corr_id of 4, or silence's unpacked modulation; tests/test_encode_ref.py --
    are left out of the PCM comparison.)"""
    pk, ft, _ = run_all()
    b = L.LPCNetBatch(S, 0, BLOB)
    x = np.ascontiguousarray(PCM.transpose(1, 0, 2).reshape(NP, S, 4, FRAME).transpose(0, 2, 1, 3))  # [6, 4, 24, 160]
    d_pcm, d_pk, d_ft = b.device_alloc(x.nbytes), b.device_alloc(NP * S * 8), b.device_alloc(NP * 4 * S * row * 4)
    b.h2d(d_pcm, x)
    b.encode_device(d_pcm, d_pk, d_ft, row, None, NP)
    b.sync()
    gpk, gft = np.zeros((NP, S, 8), np.uint8), np.zeros((NP, 4, S, row), np.float32)
    b.d2h(gpk, d_pk)
    b.d2h(gft, d_ft)
    assert gpk.tobytes() == pk.tobytes()
    assert same(gft, ft[..., :row])
    if row == NF:
        lossless = [s for s in range(S) if ((FX["unpacked"][s, :, 0] < 4) & (((gpk[:, s, 1] & 7) != 0) | (FX["unpacked"][s, :, 1] == 0))).all()]
        assert len(lossless) >= S // 2
        b2 = L.LPCNetBatch(S, 0, BLOB)
        d_a, d_b = b2.device_alloc(NP * 4 * S * FRAME * 2), b2.device_alloc(NP * 4 * S * FRAME * 2)
        b2.decode_frames(d_pk, d_a, NP)
        b2.sync()
        b2.reset()
        b2.synthesize_frames(None, d_ft, d_b, 4 * NP)
        b2.sync()
        pa, pb = np.zeros((4 * NP, S, FRAME), np.int16), np.zeros((4 * NP, S, FRAME), np.int16)
        b2.d2h(pa, d_a)
        b2.d2h(pb, d_b)
        assert pa.any()
        for s in lossless:
            assert np.array_equal(pa[:, s], pb[:, s]), FX["names"][s]
        b2.device_free(d_a)
        b2.device_free(d_b)
        b2.close()
    for d in (d_pcm, d_pk, d_ft):
        b.device_free(d)
    b.close()


def test_errors(require_gpu):
    b = L.LPCNetBatch(4, 0, L.synthetic_model(1, L.VARIANT_INT8))
    with pytest.raises(L.LPCNetError, match="codebook"):
        b.encode(pcm_of(4, 0))
    b.close()
    b = L.LPCNetBatch(4, 0)  # no model at all
    with pytest.raises(L.LPCNetError, match="model"):
        b.encode(pcm_of(4, 0))
    f = b.compute_features4(pcm_of(4, 0))
    for s in range(4):
        assert same(f[:, s], FX["ufeat"][s, 0])
    b.close()
    b = L.LPCNetBatch(4, 0, BLOB)
    d = b.device_alloc(4 * 4 * FRAME * 2 + 4 * 8 + 4 * 4 * NTF * 4)
    with pytest.raises(L.LPCNetError, match="row"):
        b.encode_device(d, d, d, 21, None, 1)
    b.device_free(d)
    b.close()
