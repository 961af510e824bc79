"""What the host-I/O wrappers of the calls beside synthesis refuse before they
reach the library: plc_predict, compute_features, burg_cepstrum, plc_update,
encode and compute_features4 of lpcnet_amd.LPCNetBatch, B = 3.  Every wrapper
raises ValueError for a wrong PCM dtype, a wrong PCM shape, a wrong ``active``
shape, a non-contiguous ``out`` and an ``out`` of the wrong dtype; the
caller's ``out`` keeps its sentinel through the refusal, and a correct call
afterwards on the same batch succeeds in place, inactive rows untouched.

plc_predict takes predictor rows, not PCM, and converts them to float32
whatever their dtype, so it has no wrong-PCM-dtype case; its input rows stand
in for the PCM in the shape case.  encode has two outputs, ``packets`` and
``features``: each is a wrapper of its own here."""
import numpy as np
import pytest

import lpcnet_amd as L

pytestmark = pytest.mark.gpu

B = 3
NF, NTF, FRAME = L.NB_FEATURES, L.NB_TOTAL_FEATURES, L.FRAME_SIZE

# wrapper -> (input shape, input dtype, out shape, out dtype)
SPECS = {
    "plc_predict": ((B, L.PLC_INPUTS), np.float32, (B, NF), np.float32),
    "compute_features": ((B, FRAME), np.int16, (B, NTF), np.float32),
    "burg_cepstrum": ((B, FRAME), np.int16, (B, L.BURG_CEPSTRUM), np.float32),
    "plc_update": ((B, FRAME), np.int16, (B, NF), np.float32),
    "encode_packets": ((B, 4 * FRAME), np.int16, (B, 8), np.uint8),
    "encode_features": ((B, 4 * FRAME), np.int16, (4, B, NTF), np.float32),
    "compute_features4": ((B, 4 * FRAME), np.int16, (4, B, NTF), np.float32),
}
KINDS = ["pcm_dtype", "pcm_shape", "active_shape", "out_noncontiguous", "out_dtype"]
CASES = [(w, k) for w in SPECS for k in KINDS if (w, k) != ("plc_predict", "pcm_dtype")]


@pytest.fixture(scope="module")
def batch(require_gpu):
    b = L.LPCNetBatch(B, 0, L.synthetic_model(1, L.VARIANT_INT8, codebooks=True, plc_small=True))
    yield b
    b.close()


def call(b, wrapper, x, active, out):
    """The wrapper's call; returns the array that must be ``out`` itself."""
    if wrapper == "encode_packets":
        return b.encode(x, active, packets=out, want_features=False)[0]
    if wrapper == "encode_features":
        return b.encode(x, active, features=out)[1]
    return getattr(b, wrapper)(x, active, out)


def good_input(wrapper):
    shape, dtype = SPECS[wrapper][:2]
    rng = np.random.default_rng(18)
    if dtype == np.float32:
        return np.zeros(shape, np.float32)
    return rng.integers(-8000, 8000, shape).astype(np.int16)


def sentinel(wrapper, dtype=None):
    shape, dt = SPECS[wrapper][2:]
    dtype = dt if dtype is None else dtype
    return np.full(shape, 0x5A if np.dtype(dtype).kind in "ui" else -77.25, dtype)


def rows(wrapper, out):
    """out as [B, ...]: the stream axis first."""
    return out if out.ndim == 2 else np.moveaxis(out, 1, 0)


@pytest.mark.parametrize("wrapper,kind", CASES)
def test_refusal_keeps_out_and_batch_usable(batch, wrapper, kind):
    shape, dtype, oshape, odtype = SPECS[wrapper]
    x, active, out = good_input(wrapper), None, sentinel(wrapper)
    bad = []  # (input, active, out) triples the wrapper must refuse
    if kind == "pcm_dtype":
        bad = [(x.astype(t), active, out) for t in (np.int32, np.float64, np.uint16)]
    elif kind == "pcm_shape":
        bad = [(x[:, :-1], active, out), (x.reshape(-1), active, out),
               (np.concatenate([x, x[:1]]), active, out)]
    elif kind == "active_shape":
        bad = [(x, np.ones(B + 1, np.uint8), out), (x, np.ones((B, 1), np.uint8), out), (x, np.ones(B - 1, bool), out)]
    elif kind == "out_noncontiguous":
        wide = np.full(oshape[:-1] + (2 * oshape[-1],), out.flat[0], odtype)
        out = wide[..., ::2]
        assert out.shape == oshape and not out.flags.c_contiguous
        bad = [(x, active, out)]
    elif kind == "out_dtype":
        other = [np.float64, np.int32] if odtype == np.float32 else [np.int8, np.float32]
        bad = [(x, active, sentinel(wrapper, t)) for t in other]
    for bx, ba, bo in bad:
        keep = bo.copy()
        with pytest.raises(ValueError):
            call(batch, wrapper, bx, ba, bo)
        assert np.array_equal(bo, keep), "a refused call wrote to the caller's out"

    # the batch still works: in place, stream 1 inactive keeps its sentinel
    good = sentinel(wrapper)
    ret = call(batch, wrapper, x, np.array([1, 0, 1], np.uint8), good)
    assert ret is good
    r = rows(wrapper, good)
    s = rows(wrapper, sentinel(wrapper))
    assert np.array_equal(r[1], s[1])
    assert not np.array_equal(r[0], s[0]) and not np.array_equal(r[2], s[2])
