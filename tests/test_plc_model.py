"""The PLC prediction network's model records (host side, no GPU): the
synthetic records and their dimensions, the load path's refusals, and the CPU
composition of compute_plc_pred (tests/plc_ref.py) that the GPU tests of
tests/test_gpu_plc_pred.py compare against."""
import hashlib

import numpy as np
import pytest

import lpcnet_amd as L
import oracle_lib as O
import plc_ref as P

NSTREAMS = 17  # the largest batch of the GPU tests


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def blob_default():
    return L.synthetic_model(1, L.VARIANT_INT8, plc=True)


@pytest.fixture(scope="module")
def blob_small():
    return L.synthetic_model(1, L.VARIANT_INT8, plc_small=True)


def test_plc_dims(blob_default, blob_small):
    assert L.plc_dims(blob_default) == (57, 128, 256, 256)
    assert L.plc_dims(blob_small) == (57, 64, 128, 64)
    # the records ride behind the codebooks and leave them alone
    both = L.synthetic_model(1, L.VARIANT_INT8, codebooks=True, plc=True)
    assert L.plc_dims(both) == (57, 128, 256, 256)
    L.validate_model(both)


# sha256 of synthetic_model(seed, variant, saturating, skewed, codebooks) as
# generated before the PLC flag bits existed: the blobs the goldens under
# tests/golden/ were made from
HEAD_BLOBS = {
    (1, 0, False, False, False): "448d469dc565f4b0daf69a31185de3547b8eef8881e0704024c795d9552ccb1e",
    (1, 1, False, False, False): "1b840861e5a6716b6cdd4cbcc7a4f21a3416e5c489265863c80079b08cd86932",
    (7, 0, True, False, False): "f9cbddb8ca090b2b9a85175eca4ab265bf30733a4bbd85e977be0717dee29cf5",
    (3, 0, False, True, False): "3965850df1e91a18af414f744c06da5618583f1e712fb61a3fad9c72efae0375",
    (1, 0, False, False, True): "ed6ec52adeb29f8a5f0f725c13baf797bc3e4cf3dfdf37d20bd8d886a95f82f9",
    (2, 1, False, False, True): "16af37df5b40cf0d0c5c71b7043d5699dd4e18b32769a98e1ce1d465ab0e42b2",
}


@pytest.mark.parametrize("args", sorted(HEAD_BLOBS))
def test_blob_without_plc_flag_is_unchanged(args):
    blob = L.synthetic_model(*args)
    L.validate_model(blob)
    assert hashlib.sha256(blob).hexdigest() == HEAD_BLOBS[args]
    # the PLC records are appended: every other array is byte-identical
    for kw in (dict(plc=True), dict(plc_small=True)):
        with_plc = L.synthetic_model(*args, **kw)
        assert with_plc[:len(blob)] == blob and len(with_plc) > len(blob)
        L.validate_model(with_plc)
    with pytest.raises(L.LPCNetError) as e:
        L.plc_dims(blob)
    assert "no PLC records" in str(e.value)


def replace_record(blob: bytes, name: str, payload: bytes) -> bytes:
    """``blob`` with the payload of record ``name`` replaced (header size and
    block length rewritten, nnet.h:54-61)."""
    off, size = P.records(blob)[name]
    block = int(np.frombuffer(blob, np.int32, 1, off - 64 + 16)[0])
    head = bytearray(blob[off - 64:off])
    nblock = (len(payload) + 63) // 64 * 64
    head[12:16] = np.int32(len(payload)).tobytes()
    head[16:20] = np.int32(nblock).tobytes()
    return blob[:off - 64] + bytes(head) + payload + bytes(nblock - len(payload)) + blob[off + block:]


def payload(blob: bytes, name: str) -> bytearray:
    off, size = P.records(blob)[name]
    return bytearray(blob[off:off + size])


def truncated(blob):
    return replace_record(blob, "plc_gru1_subias", bytes(payload(blob, "plc_gru1_subias")[:-64]))


def idx_misaligned(blob):
    idx = np.frombuffer(bytes(payload(blob, "plc_gru2_weights_idx")), np.int32).copy()
    assert idx[0] > 0
    idx[1] |= 1  # pos & 3
    return replace_record(blob, "plc_gru2_weights_idx", idx.tobytes())


def idx_past_the_end(blob):
    idx = np.frombuffer(bytes(payload(blob, "plc_gru1_weights_idx")), np.int32).copy()
    assert idx[0] > 0
    idx[1] = L.plc_dims(blob)[1]  # pos + 3 >= nb_in
    return replace_record(blob, "plc_gru1_weights_idx", idx.tobytes())


def saturating(blob):
    w = payload(blob, "plc_gru2_recurrent_weights")
    w[32 * 5 + 4 * 3 + 2] = 127  # one maddubs pair of block 5, row 3: 255 * (127 + 127) > 32767
    w[32 * 5 + 4 * 3 + 3] = 127
    return replace_record(blob, "plc_gru2_recurrent_weights", bytes(w))


def saturating_input(blob):
    w = payload(blob, "plc_gru1_weights")
    w[0] = 0x80  # -128, -128: 255 * 256 > 32768
    w[1] = 0x80
    return replace_record(blob, "plc_gru1_weights", bytes(w))


def wrong_out_rows(blob):
    return replace_record(blob, "plc_out_bias", bytes(payload(blob, "plc_out_bias")) + bytes(4))


def unsupported_units(blob):
    # 6 * 96 floats: units = 96, no multiple of 64
    return replace_record(blob, "plc_gru1_bias", bytes(24 * 96))


@pytest.mark.parametrize("damage", [truncated, idx_misaligned, idx_past_the_end, saturating, saturating_input,
                                    wrong_out_rows, unsupported_units])
def test_damaged_plc_records_are_refused(blob_small, damage):
    bad = damage(blob_small)
    with pytest.raises(L.LPCNetError) as e:
        L.plc_dims(bad)
    assert str(e.value).startswith("PLC: ") and len(str(e.value)) > 5, str(e.value)
    L.validate_model(bad)  # the synthesis part is intact
    assert L.plc_dims(blob_small) == (57, 64, 128, 64)


def test_fp32_blob_is_refused():
    blob = L.synthetic_model(1, L.VARIANT_FP32, plc=True)
    with pytest.raises(L.LPCNetError) as e:
        L.plc_dims(blob)
    assert "fp32" in str(e.value)
    L.validate_model(blob)


class _Hybrid:
    """The reference's compiled matrix kernels with the port's activations:
    everything of the composition that does not pass through the host CPU's
    rcpps (vec_avx.h:408,437), which differs between CPU vendors."""

    def __init__(self):
        ref, port = O.kernel_table(O.ref_kernels()), O.kernel_table(O.port_kernels())
        self.sgemv16, self.sparse8x4_i8, self.dense8x4_i8 = ref.sgemv16, ref.sparse8x4_i8, ref.dense8x4_i8
        self.vec_tanh, self.vec_sigmoid = port.vec_tanh, port.vec_sigmoid


@pytest.mark.parametrize("shape", ["default", "small"])
def test_composition_agrees_between_tables(blob_default, blob_small, shape):
    """The CPU composition on the port table, and where oracle/_ref is built
    on the reference's compiled table.  The two agree bit for bit where this
    CPU's rcpps is the pinned Intel table; on another CPU (an AMD host) the
    reference's activations legitimately differ (tests/test_gpu_samebox.py),
    and what must agree is the composition with the reference's compiled
    sgemv_accum16 / sparse_sgemv_accum8x4 / sgemv_accum8x4 under the port's
    activations."""
    blob = blob_default if shape == "default" else blob_small
    for s in (0, 5):
        outs, state = P.sequence(blob, s)
        assert outs.shape == (P.NCALLS, 20) and np.all(np.isfinite(outs))
        assert len(state) == 4 * sum(L.plc_dims(blob)[2:])
        if not O.have_ref():
            continue
        r = P.PlcRef(blob, _Hybrid())
        hy = np.stack([r.predict(x) for x in P.call_inputs(s)])
        assert np.array_equal(bits(hy), bits(outs)) and r.save() == state
        outs_ref, state_ref = P.sequence(blob, s, "ref")
        tab, bad = O.ref_rcp_table()
        assert np.all(np.isfinite(outs_ref))
        if bad == 0 and np.array_equal(tab, O.RCP_TABLE):
            assert np.array_equal(bits(outs_ref), bits(outs)) and state_ref == state


@pytest.mark.parametrize("shape", ["default", "small"])
def test_test_data_exercises_the_network(blob_default, blob_small, shape):
    """Conditions on the shared test data, so that the GPU parity tests cannot
    pass vacuously: the GRU states stay well inside (-1, 1) (a saturated state
    quantises to the same byte whatever the arithmetic), they move, and the
    out[19] clamp takes both branches."""
    blob = blob_default if shape == "default" else blob_small
    n1 = L.plc_dims(blob)[2]
    clamped = free = 0
    for s in range(NSTREAMS):
        outs, state = P.sequence(blob, s)
        v = np.frombuffer(state, np.float32)
        for g in (v[:n1], v[n1:]):
            assert np.mean(np.abs(g) < 0.9) >= 0.5
            assert np.mean(np.abs(g) > 1e-3) >= 0.5
        clamped += int(np.sum(outs[:, 19] == np.float32(.5)))
        free += int(np.sum(outs[:, 19] < np.float32(.5)))
    assert clamped > 0 and free > 0
    # the three input forms all occur, in every stream
    for s in range(NSTREAMS):
        forms = {"zeros" if x is None else ("fec" if x[56] < 0 else "update") for x in P.call_inputs(s)}
        assert forms == {"zeros", "fec", "update"}
