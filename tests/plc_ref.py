"""CPU reference of the PLC prediction network (compute_plc_pred,
lpcnet_plc.c:135-145), composed from the checker's kernel primitives
(oracle_lib.kernel_table: the port, or the reference's own compiled kernels),
and the test inputs shared by tests/test_plc_model.py and
tests/test_gpu_plc_pred.py.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

import lpcnet_amd as L
import oracle_lib as O

NB_BANDS = 18
NF = L.NB_FEATURES
PLC_IN = 2 * NB_BANDS + NF + 1
NCALLS = 8


def records(blob: bytes) -> dict:
    """{name: (offset of the payload, size)} of a weight blob (nnet.h:54-61 WeightHead)."""
    out, p = {}, 0
    while p < len(blob):
        size = int(np.frombuffer(blob, np.int32, 1, p + 12)[0])
        block = int(np.frombuffer(blob, np.int32, 1, p + 16)[0])
        name = blob[p + 20:p + 64].split(b"\0")[0].decode()
        out[name] = (p + 64, size)
        p += 64 + block
    return out


def _arr(blob, rec, name, dtype):
    off, size = rec[name]
    return np.frombuffer(blob, dtype, size // np.dtype(dtype).itemsize, off).copy()


class _Gru:
    def __init__(self, blob, rec, name, nin):
        self.bias = _arr(blob, rec, name + "_bias", np.float32)
        self.n = self.bias.size // 6
        self.nin = nin
        self.subias = _arr(blob, rec, name + "_subias", np.float32)
        self.w = _arr(blob, rec, name + "_weights", np.int8)
        self.idx = _arr(blob, rec, name + "_weights_idx", np.int32)
        self.rec = _arr(blob, rec, name + "_recurrent_weights", np.int8)
        assert self.subias.size == 6 * self.n and self.rec.size == 3 * self.n * self.n


class PlcRef:
    """One stream's PLCNetState and compute_plc_pred on kernel table ``k``
    (O.kernel_table(O.port_kernels()) or ...(O.ref_kernels()))."""

    def __init__(self, blob: bytes, k=None):
        self.k = k if k is not None else O.kernel_table(O.port_kernels())
        rec = records(blob)
        self.d1_b = _arr(blob, rec, "plc_dense1_bias", np.float32)
        self.cond = self.d1_b.size
        self.d1_w = _arr(blob, rec, "plc_dense1_weights", np.float32)
        assert self.d1_w.size == PLC_IN * self.cond
        self.g1 = _Gru(blob, rec, "plc_gru1", self.cond)
        self.g2 = _Gru(blob, rec, "plc_gru2", self.g1.n)
        self.out_b = _arr(blob, rec, "plc_out_bias", np.float32)
        self.out_w = _arr(blob, rec, "plc_out_weights", np.float32).reshape(self.g2.n, NF)
        assert self.out_b.size == NF
        self.reset()

    def reset(self):
        self.s1 = np.zeros(self.g1.n, np.float32)
        self.s2 = np.zeros(self.g2.n, np.float32)

    def save(self) -> bytes:
        return self.s1.tobytes() + self.s2.tobytes()

    def restore(self, st: bytes):
        v = np.frombuffer(st, np.float32)
        self.s1, self.s2 = v[:self.g1.n].copy(), v[self.g1.n:].copy()

    def _gru(self, g: _Gru, state: np.ndarray, x: np.ndarray) -> np.ndarray:
        """compute_gruB (nnet.c:326-372, DOT_PROD / USE_SU_BIAS) with a zero condition."""
        k, n = self.k, g.n
        x = np.ascontiguousarray(x, np.float32)
        state = np.ascontiguousarray(state, np.float32)
        zrh = (g.subias[:3 * n] + np.zeros(3 * n, np.float32)).astype(np.float32)
        k.sparse8x4_i8(zrh.ctypes.data, g.w.ctypes.data, 3 * n, g.nin, g.idx.ctypes.data, x.ctypes.data)
        recur = g.subias[3 * n:].copy()
        k.dense8x4_i8(recur.ctypes.data, g.rec.ctypes.data, 3 * n, n, state.ctypes.data)
        zrh[:2 * n] += recur[:2 * n]
        zr = np.ascontiguousarray(zrh[:2 * n])
        k.vec_sigmoid(zr.ctypes.data, zr.ctypes.data, 2 * n)
        z, r = zr[:n], zr[n:]
        h = zrh[2 * n:] + recur[2 * n:] * r
        h = np.ascontiguousarray(h, np.float32)
        k.vec_tanh(h.ctypes.data, h.ctypes.data, n)
        hook = getattr(self, "gru_hook", None)  # tests/tile_cases.py reads the gates from the composition
        if hook is not None:
            hook(g, x, state, z, r, h)
        return (z * state + (np.float32(1) - z) * h).astype(np.float32)

    def predict(self, x: np.ndarray | None = None) -> np.ndarray:
        """out[20] for the 57 inputs ``x`` (None: the all-zero concealment input)."""
        k = self.k
        x = np.zeros(PLC_IN, np.float32) if x is None else np.ascontiguousarray(x, np.float32)
        d = self.d1_b.copy()
        k.sgemv16(d.ctypes.data, self.d1_w.ctypes.data, self.cond, PLC_IN, self.cond, x.ctypes.data)
        k.vec_tanh(d.ctypes.data, d.ctypes.data, self.cond)
        self.s1 = self._gru(self.g1, self.s1, d)
        self.s2 = self._gru(self.g2, self.s2, self.s1)
        # plc_out has 20 rows: the generic loop of sgemv_accum (nnet.c:80-84),
        # a separate multiply and add per column in index order
        o = self.out_b.copy()
        for j in range(self.g2.n):
            o += self.out_w[j] * self.s2[j]
        v = np.float32(o[NF - 1] + np.float32(.1))
        o[NF - 1] = np.float32(.5) if np.float32(.5) < v else v
        return o


def call_inputs(stream: int, ncalls: int = NCALLS) -> list:
    """The inputs of ``ncalls`` consecutive predictor calls of one stream, a
    mix of the reference's three forms that differs from stream to stream:
    None (zeros: conceal, lpcnet_plc.c:161-162), the FEC form (features at
    [36, 56), flag -1, :156-158) and the update form (Burg cepstrum, features,
    flag +1, :206-209 / :252-255)."""
    feats = L.synthetic_features(1000 + stream, ncalls)[:, :NF]
    rng = np.random.RandomState(4242 + stream)
    forms = ["update", "update", "zeros", "fec", "zeros", "update", "fec", "zeros"]
    out = []
    for c in range(ncalls):
        form = forms[(c + 3 * stream) % len(forms)]
        if form == "zeros":
            out.append(None)
            continue
        x = np.zeros(PLC_IN, np.float32)
        x[2 * NB_BANDS:2 * NB_BANDS + NF] = feats[c]
        if form == "fec":
            x[PLC_IN - 1] = -1
        else:
            x[:2 * NB_BANDS] = (0.5 * rng.randn(2 * NB_BANDS)).astype(np.float32)
            x[PLC_IN - 1] = 1
        out.append(x)
    return out


def batch_inputs(nstreams: int, call: int) -> np.ndarray:
    """[B, 57] inputs of call ``call`` (a zeros-form stream has a zero row)."""
    x = np.zeros((nstreams, PLC_IN), np.float32)
    for s in range(nstreams):
        v = call_inputs(s)[call]
        if v is not None:
            x[s] = v
    return x


_SEQ = {}


def sequence(blob: bytes, stream: int, table: str = "port"):
    """(outs [NCALLS, 20], final state bytes) of the NCALLS-call sequence of
    one stream from reset, computed once per (blob, stream, table)."""
    key = (hash(blob), len(blob), stream, table)
    if key not in _SEQ:
        k = O.kernel_table(O.ref_kernels() if table == "ref" else O.port_kernels())
        r = PlcRef(blob, k)
        outs = np.stack([r.predict(x) for x in call_inputs(stream)])
        outs.setflags(write=False)
        _SEQ[key] = (outs, r.save())
    return _SEQ[key]
