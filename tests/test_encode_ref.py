"""CPU checks of the 1.6 kb/s encoder's reference (tests/enc_packet_ref.py, a
float32 numpy restatement of lpcnet_enc.c:53-400, 579-743, 872-909 around the
reference's compiled freq.c / pitch.c) and of the host-only main_pitch
evaluation the encoder kernel shares.

PARITY UNPINNED by a reference build of lpcnet_enc.c (nnet_data.h and
ceps_codebooks.c are generated and absent); the restatement is checked
against the decoder oracle (oracle_decode_packet), which it shares no code
with: what the encoder says it quantised is what the decoder reconstructs."""
import importlib.util
import math
import os

import numpy as np
import pytest

import enc_packet_ref as P
import feat_signals as FS
import lpcnet_amd as L
import oracle_lib as O

F = np.float32
needs_ref = pytest.mark.skipif(not P.E.have_ref(), reason="oracle/_ref (the reference's compiled kernels) not built")
BLOB = L.synthetic_model(1, L.VARIANT_INT8, codebooks=True)


def fields(packets: np.ndarray) -> np.ndarray:
    """[..., 8] packets -> [..., 9] fields in P.FIELDS order."""
    flat = packets.reshape(-1, 8)
    return np.array([list(P.unpack(p).values()) for p in flat]).reshape(packets.shape[:-1] + (9,))


def test_fixture_shapes_and_codebooks():
    fx = P.fixture()
    S = len(fx["names"])
    assert S == 24 and fx["names"][-1] == "zero" and not fx["pcm"][-1].any()
    assert fx["pcm"].shape == (S, 24, 160) and fx["pcm"].dtype == np.int16
    assert fx["packets"].shape == fx["tie_packets"].shape == (S, 6, 8)
    assert fx["qfeat"].shape == fx["ufeat"].shape == (S, 6, 4, 36)
    assert fx["state_enc"].shape == fx["state_feat"].shape == fx["mix_state"].shape == (S, FS.STATE_SIZE + 4 * P.NB)
    cb = P.blob_codebooks(BLOB)
    for k, v in P.fixture_codebooks().items():
        assert np.array_equal(v.view(np.uint32), cb[k].view(np.uint32)), k


def test_reference_agrees_with_decoder_oracle():
    """decode_packet of every reference packet, chained through vq_mem, gives
    the reference's quantised cepstrum, pitch and correlation (20 values x 4
    frames) bit for bit -- but for the two places where the reference's packet
    carries less than its encoder's own st->features use, both the
    reference's behaviour (lpcnet_enc.c:668, 687-691 against 727-728):

      * corr_id = 4 (frame_corr of 1 or more, voiced; or next to .3, unvoiced)
        packs as 0, so the decoder's correlation is corr_id 0's;
      * an unvoiced packet packs 0 for the modulation, while the encoder's own
        pitch uses the modulation it found, which is not 0 when center_pitch
        is NaN (digital silence: sw = 0, (int)NaN = INT_MIN, clamped to -3).

    There the decoder's value must be the reference formula's for what the
    packet carries; everything else is equal.  Both cases occur in the fixture."""
    fx = P.fixture()
    lost_corr = lost_mod = 0
    for s in range(len(fx["names"])):
        o = O.Oracle(BLOB)
        for p in range(P.NPACKETS):
            got = o.decode_packet(bytes(fx["packets"][s, p]))[:, :20]
            want = fx["qfeat"][s, p, :, :20].copy()
            f = P.unpack(fx["packets"][s, p])
            corr_id, modulation = (int(v) for v in fx["unpacked"][s, p])
            voiced = f["modulation"] != 0
            assert f["corr_id"] == corr_id & 3 and (f["modulation"] == modulation + 4 if voiced else True)
            if corr_id != f["corr_id"]:
                assert corr_id == 4
                fc = F(F(0.3875) + F(F(.175) * F(0))) if voiced else F(F(0.0375) + F(F(.075) * F(0)))
                want[:, 19] = F(fc - F(.5))
                lost_corr += 1
            if not voiced and modulation != 0:
                assert f["main_pitch"] == 0 and modulation == -3
                for sub in range(4):
                    pp = F(math.pow(2.0, f["main_pitch"] / 21.) * 32)
                    pp = F(pp * F(F(1) + F(F(F(F(0) / F(16)) / F(7)) * F(2 * sub - 3))))
                    pp = min(F(255), max(F(33), pp))
                    want[sub, 18] = F(F(.02) * F(pp - F(100)))
                lost_mod += 1
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (s, p)
    assert lost_corr and lost_mod


def test_fixture_coverage():
    fx = P.fixture()
    f = fields(fx["packets"])
    voiced = f[..., 2] != 0
    assert voiced.any() and (~voiced).any()
    assert (f[..., 7] >= 4096).any() and (f[..., 7] < 4096).any()
    assert len(set((f[..., 7] & 3).ravel().tolist())) >= 3
    assert len(set(f[..., 8].ravel().tolist())) >= 4
    assert (f[..., 4] != fx["nearest1"]).any()  # a winning path not built on the first stage's nearest entry
    assert (f[-1, :, 1] == 0).all() and (f[-1, :, 2] == 0).all()  # silence: main_pitch 0, unvoiced
    # the tie codebooks change the answer somewhere, and ties put the earlier index first
    tf = fields(fx["tie_packets"])
    assert (tf[..., 4:7] < 512).all() and ((tf[..., 7] & 4095) < 2048).all()


def python_thresholds() -> np.ndarray:
    """The smallest float32 center_pitch that reaches main_pitch m, m = 1..63,
    by bisection over bit patterns with Python's math.log."""
    out = []
    for m in range(1, 64):
        lo, hi = 0x00800000, 0x7f7fffff
        while hi - lo > 1:
            mid = (lo + hi) // 2
            v = np.array([mid], np.uint32).view(F)[0]
            if P.dfloor(.5 + 21. * 1.442695041 * P.dlog(float(F(v) / F(32)))) >= m:
                hi = mid
            else:
                lo = mid
        out.append(hi)
    return np.array(out, np.uint32)


def test_enc_main_pitch_matches_the_reference_expression():
    thr = python_thresholds()
    assert (np.diff(thr.astype(np.int64)) > 0).all()
    rng = np.random.RandomState(20261020)
    x = np.concatenate([
        (thr - 1).view(F), thr.view(F), (thr + 1).view(F),
        rng.uniform(16, 600, 100000).astype(F),
        np.array([0, -0.0, -1, -32, 1e-45, 1e-39, -1e-40, 1.17549435e-38, np.inf, -np.inf, np.nan, 3.4e38, 32, 31.999998], F),
    ])
    got = L.enc_main_pitch(x)
    want = np.array([P.main_pitch_of(v) for v in x], np.int32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (x[bad][:8], got[bad][:8], want[bad][:8])
    assert got.min() == 0 and got.max() == 63 and set(got[63:126].tolist()) == set(range(1, 64))


@needs_ref
def test_fixture_regenerates():
    spec = importlib.util.spec_from_file_location(
        "make_enc_packet_golden", os.path.join(os.path.dirname(P.GOLDEN), "make_enc_packet_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    a, fx = m.arrays(), P.fixture()
    assert set(a) == set(fx)
    for k, v in a.items():
        assert v.dtype == fx[k].dtype and v.shape == fx[k].shape, k
        assert v.tobytes() == fx[k].tobytes(), k
