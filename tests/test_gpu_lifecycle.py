"""A batch's lifecycle across models: a second model with other dimensions is
loaded onto a batch whose lazily allocated side buffers (extractor, Burg,
encoder, RDO-VAE state, decode staging) already exist, the kernel mode is
changed and changed back, and every family must then compute what a fresh
batch computes: the predictor and the RDO-VAE against their CPU compositions
(tests/plc_ref.py, tests/rdovae_ref.py) bit for bit, synthesis against the
golden fixture.  Three such cycles of create, load, use, close in one process
must give the same bits."""
import os

import numpy as np
import pytest

import lpcnet_amd as L
import oracle_lib as O
import plc_ref as P
import rdovae_ref as R

pytestmark = pytest.mark.gpu

NF = L.NB_FEATURES
GOLDEN_FRAMES = 6

_CACHE = {}


def blobs():
    if not _CACHE:
        _CACHE["first"] = L.synthetic_model(1, L.VARIANT_INT8, codebooks=True, plc=True, rdovae=True)
        _CACHE["second"] = L.synthetic_model(1, L.VARIANT_INT8, codebooks=True, plc_small=True, rdovae_small=True)
        _CACHE["golden"] = np.load(os.path.join(O.GOLDEN, "streams_int8.npz"))
    return _CACHE["first"], _CACHE["second"], _CACHE["golden"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dec_inputs(blob, B):
    d = L.rdovae_dims(blob)["dec"]
    st = np.stack([R.dec_state(s, d["S"]) for s in range(B)])
    z = np.stack([R.dec_latents(s, d["L"]) for s in range(B)])
    return st, z


def touch(b, B, blob, G):
    """One call of each family; everything they returned, as bytes."""
    pcm = (3000 * np.random.RandomState(B).randn(B, 4 * 160)).astype(np.int16)
    st, z = dec_inputs(blob, B)
    out = [b.plc_predict(P.batch_inputs(B, 0)), b.compute_features(pcm[:, :160]), b.burg_cepstrum(pcm[:, 160:320])]
    out += list(b.encode(pcm))
    out += list(b.rdovae_encode(R.enc_batch(B, 0)))
    b.rdovae_dec_init(st)
    out.append(b.rdovae_decode_qframe(z[:, 0]))
    out.append(b.synthesize(G["features"][np.arange(B) % len(G["streams"]), 0, :NF]))
    assert all(np.asarray(o).size for o in out) and any(np.any(np.asarray(o)) for o in out)
    return [np.asarray(o).tobytes() for o in out]


def cycle(B):
    first, second, G = blobs()
    b = L.LPCNetBatch(B, 0, first)
    outs = touch(b, B, first, G)
    # the second model, with other PLC and RDO-VAE dimensions, on the same batch
    b.load_model(second)
    b.set_kernel(1)
    b.set_kernel(0)
    assert b.plc_info() == L.plc_dims(second) and b.rdovae_info() == L.rdovae_dims(second)
    for c in range(P.NCALLS):
        x = P.batch_inputs(B, c)
        o = b.plc_predict(x)
        outs.append(o.tobytes())
        for s in range(B):
            assert np.array_equal(bits(o[s]), bits(P.sequence(second, s)[0][c])), ("plc", c, s)
    for s in range(B):
        assert b.plc_save_state(s) == bytes(P.sequence(second, s)[1]), ("plc state", s)
    for c in range(R.NENC):
        z, st = b.rdovae_encode(R.enc_batch(B, c))
        outs += [z.tobytes(), st.tobytes()]
        for s in range(B):
            ref = R.enc_sequence(second, s)
            assert np.array_equal(bits(z[s]), bits(ref[0][c])) and np.array_equal(bits(st[s]), bits(ref[1][c])), ("enc", c, s)
    st, z = dec_inputs(second, B)
    b.rdovae_dec_init(st)
    for c in range(R.NDEC):
        q = b.rdovae_decode_qframe(z[:, c])
        outs.append(q.tobytes())
        for s in range(B):
            assert np.array_equal(bits(q[s]), bits(R.dec_sequence(second, s)[0][c])), ("dec", c, s)
    for s in range(B):
        assert b.rdovae_save_state(s, 1) == bytes(R.enc_sequence(second, s)[2]), ("enc state", s)
        assert b.rdovae_save_state(s, 2) == bytes(R.dec_sequence(second, s)[1]), ("dec state", s)
    # a load keeps the streams' synthesis state: from reset, the golden fixture's frames
    b.reset()
    idx = np.arange(B) % len(G["streams"])
    for fr in range(GOLDEN_FRAMES):
        pcm = b.synthesize(G["features"][idx, fr, :NF])
        outs.append(pcm.tobytes())
        assert np.array_equal(pcm, G["pcm"][idx, fr]), ("synthesis", fr)
    # the families whose buffers outlived the load still run
    outs += touch(b, B, second, G)
    b.close()
    return outs


@pytest.mark.parametrize("B", [3, 17])
def test_second_model_on_a_used_batch(require_gpu, B):
    """B = 3: a partial 16-stream tile; 17: a second tile of one stream."""
    runs = [cycle(B) for _ in range(3)]
    assert runs[2] == runs[0]
