"""CPU reference of the DRED RDO-VAE (dred_rdovae_enc.c:38-95
dred_rdovae_encode_dframe, dred_rdovae_dec.c:37-98 dec_init_states /
decode_qframe, dred_rdovae.c:38-52 DRED_rdovae_decode_all), composed from the
checker's kernel primitives (oracle_lib.kernel_table: the port, or the
reference's own compiled kernels), and the test inputs shared by
tests/test_rdovae_model.py and tests/test_gpu_rdovae.py.
TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

import lpcnet_amd as L
import oracle_lib as O
import plc_ref as P

NF = L.NB_FEATURES
QFRAME = 4 * NF
NENC = 6  # encoder calls of a sequence: the 4-tap conv memory has wrapped completely
NDEC = 4  # qframes of a decoder sequence

records, _arr, _Gru = P.records, P._arr, P._Gru


class _Dense:
    def __init__(self, blob, rec, name, nin=None):
        self.name = name
        self.b = _arr(blob, rec, name + "_bias", np.float32)
        self.out = self.b.size
        w = _arr(blob, rec, name + "_weights", np.float32)
        self.nin = w.size // self.out if nin is None else nin
        assert w.size == self.nin * self.out, name
        self.w = w.reshape(self.nin, self.out)
        self.fma = self.out % 16 == 0  # sgemv_accum (nnet.c:73-86): sgemv_accum16, or the generic loop


class _Net:
    """The stack both sides share, on kernel table ``k``."""

    def __init__(self, blob: bytes, pre: str, in_dim: int | None, k=None):
        self.k = k if k is not None else O.kernel_table(O.port_kernels())
        self.rec = rec = records(blob)
        self.blob = blob
        self.forms = set()  # the row forms the dense / conv layers took
        self.layers = []
        nin = in_dim
        for l in range(1, 9):
            name = pre + str(l)
            if l in (2, 4, 6):
                g = _Gru(blob, rec, name, nin)
                self.layers.append(g)
                nin = g.n
            else:
                d = _Dense(blob, rec, name, nin)
                self.layers.append(d)
                nin = d.out
        self.in_dim = self.layers[0].nin
        self.grus = [self.layers[i] for i in (1, 3, 5)]
        self.T = sum(l.n if isinstance(l, _Gru) else l.out for l in self.layers)
        self.states = [np.zeros(g.n, np.float32) for g in self.grus]

    _gru = P.PlcRef._gru

    def dense(self, d: _Dense, x: np.ndarray, tanh: bool = True) -> np.ndarray:
        """_lpcnet_compute_dense / the product of compute_conv1d (nnet.c:117-129, 452-470)."""
        x = np.ascontiguousarray(x, np.float32)
        assert x.size == d.nin, d.name
        o = d.b.copy()
        if d.fma:
            self.k.sgemv16(o.ctypes.data, d.w.ctypes.data, d.out, d.nin, d.out, x.ctypes.data)
        else:
            # a separate float32 multiply and add per column, in index order
            for j in range(d.nin):
                o += d.w[j] * x[j]
        self.forms.add((d.name, "fma" if d.fma else "generic"))
        if tanh:
            self.k.vec_tanh(o.ctypes.data, o.ctypes.data, d.out)
        return o

    def stack(self, x: np.ndarray) -> np.ndarray:
        """The eight layers on input ``x``; returns the concatenation [T]."""
        parts, g = [], 0
        for layer in self.layers:
            if isinstance(layer, _Gru):
                self.states[g] = self._gru(layer, self.states[g], x)
                x = self.states[g]
                g += 1
            else:
                x = self.dense(layer, x)
            parts.append(x)
        return np.concatenate(parts).astype(np.float32)

    def gru_bytes(self) -> bytes:
        return b"".join(s.tobytes() for s in self.states)


class RdoEnc(_Net):
    """One stream's RDOVAEEncState and dred_rdovae_encode_dframe."""

    def __init__(self, blob: bytes, k=None):
        super().__init__(blob, "enc_dense", 2 * NF, k)
        rec = self.rec
        self.L = _arr(blob, rec, "bits_dense_bias", np.float32).size
        self.conv = _Dense(blob, rec, "bits_dense")
        assert self.conv.nin % self.T == 0
        self.ksize = self.conv.nin // self.T
        self.g1 = _Dense(blob, rec, "gdense1", self.T)
        self.g2 = _Dense(blob, rec, "gdense2", self.g1.out)
        self.S = self.g2.out
        self.mem = np.zeros((self.ksize - 1) * self.T, np.float32)

    def encode(self, x: np.ndarray):
        """(latents [L], initial_state [S]) of the 40 inputs ``x``."""
        buf = self.stack(x)
        tmp = np.concatenate([self.mem, buf])
        z = self.dense(self.conv, tmp, tanh=False)
        self.mem = tmp[self.T:].copy()
        return z, self.dense(self.g2, self.dense(self.g1, buf))

    def save(self) -> bytes:
        return self.gru_bytes() + self.mem.tobytes()

    def restore(self, st: bytes):
        v, p = np.frombuffer(st, np.float32), 0
        for i, g in enumerate(self.grus):
            self.states[i] = v[p:p + g.n].copy()
            p += g.n
        assert v.size - p == self.mem.size
        self.mem = v[p:].copy()


class RdoDec(_Net):
    """One stream's RDOVAEDecState, dec_init_states and decode_qframe."""

    def __init__(self, blob: bytes, k=None):
        super().__init__(blob, "dec_dense", None, k)
        self.L = self.in_dim
        self.st = [_Dense(blob, self.rec, "state%d" % (i + 1)) for i in range(3)]
        self.S = self.st[0].nin
        self.final = _Dense(blob, self.rec, "dec_final", self.T)
        assert self.final.out == QFRAME

    def init(self, state: np.ndarray):
        self.states = [self.dense(d, state) for d in self.st]

    def qframe(self, z: np.ndarray) -> np.ndarray:
        return self.dense(self.final, self.stack(z), tanh=False)

    def save(self) -> bytes:
        return self.gru_bytes()

    def restore(self, st: bytes):
        v, p = np.frombuffer(st, np.float32), 0
        for i, g in enumerate(self.grus):
            self.states[i] = v[p:p + g.n].copy()
            p += g.n


def decode_all(blob: bytes, state: np.ndarray, latents: np.ndarray, k=None) -> np.ndarray:
    """DRED_rdovae_decode_all: a temporary zeroed state, dec_init, one qframe
    per latent; latent i writes features[80 i .. 80 i + 80).  Returns [4 n, 20]."""
    d = RdoDec(blob, k)
    d.init(state)
    return np.concatenate([d.qframe(z) for z in latents]).reshape(-1, NF)


# ---- deterministic per-stream inputs ----------------------------------------
def enc_inputs(stream: int, ncalls: int = NENC) -> np.ndarray:
    """[ncalls, 40]: consecutive pairs of synthetic feature frames, the earlier first."""
    f = L.synthetic_features(2000 + stream, 2 * ncalls)[:, :NF]
    return np.ascontiguousarray(f.reshape(ncalls, 2 * NF))


def enc_batch(nstreams: int, call: int) -> np.ndarray:
    return np.stack([enc_inputs(s)[call] for s in range(nstreams)])


# The synthetic encoders' latents have a standard deviation near 0.75 and their
# initial states fill (-1, 1) (tests/test_rdovae_model.py checks both): the
# decoder's test inputs are drawn in that range.
def dec_state(stream: int, S: int) -> np.ndarray:
    return np.random.RandomState(7000 + stream).uniform(-0.9, 0.9, S).astype(np.float32)


def dec_latents(stream: int, Ld: int, n: int = NDEC) -> np.ndarray:
    return (0.75 * np.random.RandomState(9000 + stream).randn(n, Ld)).astype(np.float32)


def _table(table: str):
    return O.kernel_table(O.ref_kernels() if table == "ref" else O.port_kernels())


_SEQ = {}


def enc_sequence(blob: bytes, stream: int, table: str = "port"):
    """(latents [NENC, L], states [NENC, S], final state bytes, the encoder)
    of the NENC-call sequence of one stream from reset, computed once per
    (blob, stream, table)."""
    key = ("enc", hash(blob), len(blob), stream, table)
    if key not in _SEQ:
        e = RdoEnc(blob, _table(table))
        out = [e.encode(x) for x in enc_inputs(stream)]
        z, st = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
        z.setflags(write=False)
        st.setflags(write=False)
        _SEQ[key] = (z, st, e.save(), e)
    return _SEQ[key]


def dec_sequence(blob: bytes, stream: int, table: str = "port"):
    """(qframes [NDEC, 80], final state bytes, the decoder) of dec_init and
    NDEC qframes of one stream, computed once per (blob, stream, table)."""
    key = ("dec", hash(blob), len(blob), stream, table)
    if key not in _SEQ:
        d = RdoDec(blob, _table(table))
        d.init(dec_state(stream, d.S))
        q = np.stack([d.qframe(z) for z in dec_latents(stream, d.L)])
        q.setflags(write=False)
        _SEQ[key] = (q, d.save(), d)
    return _SEQ[key]


def all_sequence(blob: bytes, stream: int, n: int, table: str = "port") -> np.ndarray:
    """decode_all [4 n, 20] of the stream's state and first n latents."""
    key = ("all", hash(blob), len(blob), stream, n, table)
    if key not in _SEQ:
        d = dec_sequence(blob, stream, table)[2]
        f = decode_all(blob, dec_state(stream, d.S), dec_latents(stream, d.L)[:n], _table(table))
        f.setflags(write=False)
        _SEQ[key] = f
    return _SEQ[key]
