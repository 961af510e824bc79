"""The DRED RDO-VAE's model records (host side, no GPU): the synthetic
records and their dimensions, the load path's refusals, and the CPU
composition (tests/rdovae_ref.py) that the GPU tests of
tests/test_gpu_rdovae.py compare against."""
import itertools

import numpy as np
import pytest

import lpcnet_amd as L
import oracle_lib as O
import plc_ref as P
import rdovae_ref as R
from test_plc_model import payload, replace_record

NSTREAMS = 17  # the largest batch of the GPU tests

DEFAULT = dict(L=80, S=24, T=2048, widths=(256,) * 8)
SMALL = dict(L=40, S=32, T=704, widths=(128, 64, 128, 64, 128, 64, 64, 64))
ENC_NAMES = ["enc_dense%d" % l for l in range(1, 9)] + ["bits_dense", "gdense1", "gdense2"]
DEC_NAMES = ["state1", "state2", "state3"] + ["dec_dense%d" % l for l in range(1, 9)] + ["dec_final"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def blob_default():
    return L.synthetic_model(1, L.VARIANT_INT8, rdovae=True)


@pytest.fixture(scope="module")
def blob_small():
    return L.synthetic_model(1, L.VARIANT_INT8, rdovae_small=True)


def layer_of(record: str) -> str:
    for suf in ("_recurrent_weights", "_weights_idx", "_weights", "_subias", "_bias"):
        if record.endswith(suf):
            return record[:-len(suf)]
    return record


def strip(blob: bytes, layers) -> bytes:
    """``blob`` without the records of ``layers``."""
    out, p = bytearray(), 0
    while p < len(blob):
        block = int(np.frombuffer(blob, np.int32, 1, p + 16)[0])
        name = blob[p + 20:p + 64].split(b"\0")[0].decode()
        if layer_of(name) not in layers:
            out += blob[p:p + 64 + block]
        p += 64 + block
    return bytes(out)


def test_rdovae_dims(blob_default, blob_small):
    d = L.rdovae_dims(blob_default)
    assert d == {"enc": dict(DEFAULT, kernel=4, gdense1=128), "dec": DEFAULT}
    d = L.rdovae_dims(blob_small)
    assert d == {"enc": dict(SMALL, kernel=4, gdense1=64), "dec": SMALL}
    # the records ride behind the codebooks and the PLC's and leave them alone
    all_of = L.synthetic_model(1, L.VARIANT_INT8, codebooks=True, plc=True, rdovae=True)
    assert L.rdovae_dims(all_of) == L.rdovae_dims(blob_default)
    assert L.plc_dims(all_of) == (57, 128, 256, 256)
    L.validate_model(all_of)


@pytest.mark.parametrize("flags", list(itertools.product([0, 1], [0, 1], [0, 1], ["", "plc", "plc_small"])))
def test_the_flag_only_appends_records(flags):
    """Every blob made with the earlier flags is a byte-identical prefix of
    the one with the RDO-VAE flag (tests/test_plc_model.py pins those blobs'
    hashes); plc_dims and side_digest do not see the new records."""
    sat, skew, cb, plc = flags
    kw = dict(saturating=bool(sat), skewed=bool(skew), codebooks=bool(cb), plc=plc == "plc", plc_small=plc == "plc_small")
    blob = L.synthetic_model(1, L.VARIANT_INT8, **kw)
    with pytest.raises(L.LPCNetError) as e:
        L.rdovae_dims(blob)
    assert "carries no enc_dense1..8 records" in str(e.value) and "carries no dec_dense1..8 records" in str(e.value)
    for rk in (dict(rdovae=True), dict(rdovae_small=True)):
        more = L.synthetic_model(1, L.VARIANT_INT8, **kw, **rk)
        assert more[:len(blob)] == blob and len(more) > len(blob)
        added = set(P.records(more)) - set(P.records(blob))
        assert {layer_of(n) for n in added} == set(ENC_NAMES + DEC_NAMES)
        L.validate_model(more)
        assert L.side_digest(more) == L.side_digest(blob)
        if plc:
            assert L.plc_dims(more) == L.plc_dims(blob)
        else:
            with pytest.raises(L.LPCNetError):
                L.plc_dims(more)


def test_fp32_blob_keeps_its_prefix_and_is_refused():
    blob = L.synthetic_model(1, L.VARIANT_FP32)
    more = L.synthetic_model(1, L.VARIANT_FP32, rdovae_small=True)
    assert more[:len(blob)] == blob
    L.validate_model(more)
    with pytest.raises(L.LPCNetError) as e:
        L.rdovae_dims(more)
    assert "fp32" in str(e.value)


# ---- damaged records ---------------------------------------------------------
def truncated(blob):
    return replace_record(blob, "enc_dense2_subias", bytes(payload(blob, "enc_dense2_subias")[:-64])), "enc"


def missing(blob):
    return strip(blob, {"gdense1"}), "enc"


def missing_dec(blob):
    return strip(blob, {"state2"}), "dec"


def idx_misaligned(blob):
    idx = np.frombuffer(bytes(payload(blob, "dec_dense4_weights_idx")), np.int32).copy()
    assert idx[0] > 0
    idx[1] |= 1
    return replace_record(blob, "dec_dense4_weights_idx", idx.tobytes()), "dec"


def saturating(blob):
    w = payload(blob, "enc_dense6_recurrent_weights")
    w[32 * 5 + 4 * 3 + 2] = 127
    w[32 * 5 + 4 * 3 + 3] = 127
    return replace_record(blob, "enc_dense6_recurrent_weights", bytes(w)), "enc"


def saturating_input(blob):
    w = payload(blob, "dec_dense2_weights")
    w[0] = 0x80
    w[1] = 0x80
    return replace_record(blob, "dec_dense2_weights", bytes(w)), "dec"


def producer_mismatch(blob):
    # dense3 with one more row than GRU 4 has inputs
    b = replace_record(blob, "enc_dense3_bias", bytes(payload(blob, "enc_dense3_bias")) + bytes(4))
    return b, "enc"


def gru_input_not_64(blob):
    # dec_dense1 of 96 rows: consistent records, no multiple of 64
    n = L.rdovae_dims(blob)["dec"]["L"]
    b = replace_record(blob, "dec_dense1_bias", bytes(4 * 96))
    return replace_record(b, "dec_dense1_weights", bytes(4 * 96 * n)), "dec"


def final_not_80(blob):
    T = L.rdovae_dims(blob)["dec"]["T"]
    b = replace_record(blob, "dec_final_bias", bytes(4 * 64))
    return replace_record(b, "dec_final_weights", bytes(4 * 64 * T)), "dec"


def conv_not_whole_taps(blob):
    return replace_record(blob, "bits_dense_weights", bytes(payload(blob, "bits_dense_weights")[:-4])), "enc"


def state_layer_width(blob):
    S = L.rdovae_dims(blob)["dec"]["S"]
    b = replace_record(blob, "state3_bias", bytes(4 * 128))
    return replace_record(b, "state3_weights", bytes(4 * 128 * S)), "dec"


@pytest.mark.parametrize("damage", [truncated, missing, missing_dec, idx_misaligned, saturating, saturating_input,
                                    producer_mismatch, gru_input_not_64, final_not_80, conv_not_whole_taps,
                                    state_layer_width])
def test_damaged_records_are_refused(blob_small, damage):
    bad, side = damage(blob_small)
    other = "dec" if side == "enc" else "enc"
    d = L.rdovae_dims(bad)
    good = L.rdovae_dims(blob_small)
    assert d[side] is None and d[other] == good[other]  # the sides are independent
    # the reason, once the other side is gone too
    with pytest.raises(L.LPCNetError) as e:
        L.rdovae_dims(strip(bad, set(DEC_NAMES if side == "enc" else ENC_NAMES)))
    who = "RDO-VAE encoder: " if side == "enc" else "RDO-VAE decoder: "
    msg = [m for m in str(e.value).split("; ") if m.startswith(who)]
    assert msg and "carries no" not in msg[0] and len(msg[0]) > len(who), str(e.value)
    L.validate_model(bad)  # the synthesis part is intact


def test_one_sided_blobs(blob_small):
    good = L.rdovae_dims(blob_small)
    enc_only = strip(blob_small, set(DEC_NAMES))
    dec_only = strip(blob_small, set(ENC_NAMES))
    assert L.rdovae_dims(enc_only) == {"enc": good["enc"], "dec": None}
    assert L.rdovae_dims(dec_only) == {"enc": None, "dec": good["dec"]}
    for b in (enc_only, dec_only):
        L.validate_model(b)
    # the reference composition needs only its side's records
    z, st = R.RdoEnc(enc_only).encode(R.enc_inputs(0)[0])
    assert np.array_equal(bits(z), bits(R.enc_sequence(blob_small, 0)[0][0]))
    d = R.RdoDec(dec_only)
    d.init(R.dec_state(0, d.S))
    assert np.array_equal(bits(d.qframe(R.dec_latents(0, d.L)[0])), bits(R.dec_sequence(blob_small, 0)[0][0]))


# ---- the reference composition and its test data -----------------------------
@pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref (the reference's compiled kernels) not built")
@pytest.mark.parametrize("shape", ["default", "small"])
def test_port_and_reference_tables_agree(blob_default, blob_small, shape):
    blob = blob_default if shape == "default" else blob_small
    for s in (0, 5):
        for k in range(3):
            assert np.array_equal(bits(R.enc_sequence(blob, s)[k]) if k < 2 else R.enc_sequence(blob, s)[k],
                                  bits(R.enc_sequence(blob, s, "ref")[k]) if k < 2 else R.enc_sequence(blob, s, "ref")[k])
        assert np.array_equal(bits(R.dec_sequence(blob, s)[0]), bits(R.dec_sequence(blob, s, "ref")[0]))
        assert R.dec_sequence(blob, s)[1] == R.dec_sequence(blob, s, "ref")[1]
        assert np.array_equal(bits(R.all_sequence(blob, s, 3)), bits(R.all_sequence(blob, s, 3, "ref")))


@pytest.mark.parametrize("shape", ["default", "small"])
def test_the_test_data_exercises_the_network(blob_default, blob_small, shape):
    """Over the sequences the GPU tests use, from the reference composition
    alone: every GRU state has elements both above 0.05 and below 0.999 in
    magnitude, the latents are not all below 1e-3, the decoder's inputs lie in
    the range the encoder produces, and both row forms occur."""
    blob = blob_default if shape == "default" else blob_small
    forms = set()
    zs, sts = [], []
    for s in range(NSTREAMS):
        z, st, _, e = R.enc_sequence(blob, s)
        q, _, d = R.dec_sequence(blob, s)
        zs.append(z)
        sts.append(st)
        for g in e.states + d.states:
            a = np.abs(g)
            assert (a > 0.05).any() and (a < 0.999).any(), s
        assert np.abs(z).max() > 1e-3 and np.abs(q).max() > 1e-3
        assert np.abs(e.mem).max() > 1e-3
        forms |= {f for _, f in e.forms | d.forms}
    zs, sts = np.concatenate(zs), np.concatenate(sts)
    assert 0.5 < zs.std() < 1.0, zs.std()  # dec_latents draws with 0.75
    assert np.abs(sts).max() > 0.9 and np.abs(sts).max() < 1.0 and sts.std() > 0.4, (np.abs(sts).max(), sts.std())
    if shape == "small":
        assert forms == {"fma", "generic"}
    # between the two shapes both forms are hit on the latents and on the state
    e = R.enc_sequence(blob, 0)[3]
    want = {"default": {("bits_dense", "fma"), ("gdense2", "generic")},
            "small": {("bits_dense", "generic"), ("gdense2", "fma")}}[shape]
    assert want <= e.forms


def test_decode_all_is_init_and_qframes(blob_small):
    d = R.dec_sequence(blob_small, 3)[2]
    f = R.all_sequence(blob_small, 3, 3)
    assert f.shape == (12, L.NB_FEATURES)
    assert np.array_equal(bits(f.reshape(3, 80)), bits(R.dec_sequence(blob_small, 3)[0][:3]))
    assert d.S == 32 and d.L == 40
