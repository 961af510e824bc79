"""PLC predictor and RDO-VAE models built in Python.  TEST INFRASTRUCTURE ONLY.

plc_kernel.hip and rdovae_kernel.hip share plc_gru of gru_tile.h; the two
shapes model_gen.cpp emits for each network are built to be well behaved (GRU
widths 64 / 128 / 256, conv kernel 4, every head a multiple of 8 rows, gates
that never saturate).  ``gru`` and ``dense`` emit a layer's records in the
blob's format with a chosen width, index and weight magnitude; ``MODELS`` maps
a name to the blob of one of the edge models below, made once.  Each blob is
L.synthetic_model(1, int8) (the synthesis records the load path needs) with the
side records appended.

Numbers come from mask_models.uniform (splitmix64: integer arithmetic, the same
with any numpy), never numpy's generators.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import lpcnet_amd as L
from mask_models import uniform
from test_ingest import join, make_record, records
from test_plc_model import payload, replace_record
from test_rdovae_model import DEC_NAMES, strip

NF = L.NB_FEATURES
PLC_IN = 2 * 18 + NF + 1
QFRAME = 4 * NF
HOT_FLIP = 0.05  # of a hot GRU's recurrent signs: the rest are coherent (see gru)
SEED_BOUND = 2.0 ** 31 / (128.0 * 127.0)  # |subias| beyond this: the int32 seed of vec_avx.h:705 is out of range


def _sym(seed: int, n: int, amp: float) -> np.ndarray:
    return (2.0 * uniform(seed, n) - 1.0) * amp


def _quant_pairs(w: np.ndarray) -> np.ndarray:
    """[..., 8, 4] floats -> int8 with every adjacent pair clipped to
    |a| + |b| <= 0.992 first, as model_gen.cpp's make_sparse does: 255 (q0 + q1)
    stays inside int16, what block_may_saturate accepts."""
    p = w.reshape(w.shape[:-1] + (2, 2))
    s = np.abs(p).sum(-1, keepdims=True)
    p = np.where(s > 0.992, p * (0.992 / np.maximum(s, 1e-30)), p)
    return np.clip(np.rint(128.0 * p.reshape(w.shape)), -128, 127).astype(np.int8)


def default_rows(seed: int, nin: int, n: int) -> list:
    """Half of the input blocks of every 8-row block, as emit_plc_gru leaves out."""
    keep = uniform(seed, (3 * n // 8) * (nin // 4)).reshape(3 * n // 8, nin // 4) < 0.5
    return [[int(c) for c in np.flatnonzero(k)] for k in keep]


def gru(name: str, nin: int, n: int, seed: int, rows=None, hot: bool = False, bias_amp: float = 0.1,
        big: bool = False, dup_scale: float = 1.0) -> list:
    """The five records of one compute_gruB layer (dump_plc.py dump_gru_layer,
    as model_gen.cpp emit_plc_gru): block-sparse int8 input weights [blocks][8][4]
    with their index (per 8-row block: count, then 4 * column block; ``rows``
    lists the column blocks, duplicates allowed), recurrent weights (out_blk,
    in_blk, 8, 4), bias [2][3 n] and subias = bias - sum(q) / 128 of each half.

    hot: every weight +-64, the largest magnitude at which a same-sign pair
    passes block_may_saturate (255 * 128 <= 32767).  big: six subias entries
    of each half are moved beyond +-SEED_BOUND, both signs.  dup_scale scales
    the blocks of a row that lists a block twice (so that the sum stays int8)."""
    assert nin % 64 == 0 and n % 64 == 0
    rows = default_rows(seed, nin, n) if rows is None else rows
    assert len(rows) == 3 * n // 8 and all(0 <= c < nin // 4 for r in rows for c in r)
    nblk = sum(len(r) for r in rows)
    if hot:
        qi = np.where(uniform(seed + 1, 32 * nblk) < 0.5, -64, 64).astype(np.int8).reshape(nblk, 8, 4)
        # recurrent signs: row sign * column sign with HOT_FLIP of them flipped, the column signs those of
        # the h rows, so that a state of that sign pattern drives every gate's sum the same way and holds
        sr = np.where(uniform(seed + 4, 3 * n) < 0.5, -1, 1)
        s = sr[:, None] * sr[None, 2 * n:] * np.where(uniform(seed + 2, 3 * n * n) < HOT_FLIP, -1, 1).reshape(3 * n, n)
        qr = (64 * s).astype(np.int8).reshape(3 * n // 8, 8, n // 4, 4).transpose(0, 2, 1, 3).copy()
    else:
        amp = np.concatenate([np.full(len(r), (dup_scale if len(set(r)) < len(r) else 1.0)) for r in rows] + [np.zeros(0)])
        wi = _sym(seed + 1, 32 * nblk, 0.9 * math.sqrt(3.0 / (0.5 * nin))).reshape(nblk, 8, 4) * amp.reshape(-1, 1, 1)
        qi = _quant_pairs(wi)
        qr = _quant_pairs(_sym(seed + 2, 3 * n * n, 0.7 * math.sqrt(3.0 / n)).reshape(3 * n // 8, n // 4, 8, 4))
    idx, colsum, k = [], np.zeros(3 * n), 0
    for rb, r in enumerate(rows):
        idx.append(len(r))
        idx.extend(4 * c for c in r)
        colsum[8 * rb:8 * rb + 8] = qi[k:k + len(r)].astype(np.int64).sum((0, 2)) / 128.0
        k += len(r)
    colsum2 = qr.astype(np.int64).sum((1, 3)).reshape(3 * n) / 128.0
    bias = _sym(seed + 3, 6 * n, bias_amp).astype(np.float32)
    sub = np.concatenate([bias[:3 * n].astype(np.float64) - colsum, bias[3 * n:].astype(np.float64) - colsum2]).astype(np.float32)
    if big:
        vals = np.array([1.5, -1.5, 1.0001, -1.0001, 40.0, -40.0]) * SEED_BOUND
        for half in (0, 3 * n):
            for j, v in enumerate(vals):  # two in every gate, no two in one unit
                sub[half + (j % 3) * n + 5 + 11 * j] = np.float32(v)
        assert np.sum(np.abs(sub) * (128.0 * 127.0) >= 2.0 ** 31) == 12
    return [make_record(name + "_weights", qi.tobytes()),
            make_record(name + "_weights_idx", np.asarray(idx, np.int32).tobytes()),
            make_record(name + "_recurrent_weights", qr.tobytes()),
            make_record(name + "_bias", bias.tobytes()),
            make_record(name + "_subias", sub.tobytes())]


def dense(name: str, nin: int, out: int, seed: int, gain: float = 1.0, bias_amp: float = 0.1) -> list:
    """A dense layer's two records: weights [in][out] as nnet.c reads them,
    uniform with variance gain^2 / in, and the bias."""
    w = _sym(seed, nin * out, gain * math.sqrt(3.0 / nin)).astype(np.float32)
    return [make_record(name + "_weights", w.tobytes()),
            make_record(name + "_bias", _sym(seed + 1, out, bias_amp).astype(np.float32).tobytes())]


def _base() -> list:
    return records(L.synthetic_model(1, L.VARIANT_INT8))


def idx_rows(seed: int, nin: int, n: int) -> list:
    """default_rows with block row 1 empty, block row 2 full, and in block row
    3 (and in the last) the first listed block listed a second time."""
    rows = default_rows(seed, nin, n)
    rows[1] = []
    rows[2] = list(range(nin // 4))
    for rb in (3, len(rows) - 1):
        assert rows[rb]
        rows[rb] = rows[rb] + [rows[rb][0]]
    return rows


def plc(cond: int, n1: int, n2: int, seed: int, hot: bool = False, idx: bool = False, big: bool = False) -> bytes:
    kw = dict(hot=hot, bias_amp=4.0 if hot else 0.1, big=big)
    recs = _base()
    recs += dense("plc_dense1", PLC_IN, cond, seed, 2.0 if hot else 1.0)
    # the repeated blocks at half amplitude: their sum stays inside int8 (gru_tiles_parse refuses it otherwise)
    recs += gru("plc_gru1", cond, n1, seed + 10, rows=idx_rows(seed + 10, cond, n1) if idx else None, dup_scale=0.5, **kw)
    recs += gru("plc_gru2", n1, n2, seed + 20, rows=idx_rows(seed + 20, n1, n2) if idx else None, dup_scale=0.5, **kw)
    recs += dense("plc_out", n2, NF, seed + 30)
    ob = np.frombuffer(bytes(recs[-1][2][:4 * NF]), np.float32).copy()
    ob[NF - 1] = 0.3  # the out[19] boost's clamp at .5 is met from both sides
    recs[-1] = make_record("plc_out_bias", ob.tobytes())
    return join(recs)


def rdo_side(dec: bool, widths, Lat: int, S: int, seed: int, ksize: int = 0, gdense1: int = 0, hot: bool = False) -> list:
    """One side's records: the eight-layer stack (dense1, GRU2, dense3, GRU4,
    dense5, GRU6, dense7, dense8 of ``widths``) and its heads."""
    pre = "dec_dense" if dec else "enc_dense"
    g = 6.0 if hot else 2.0  # hot: the dense layers' tanh reaches exactly +-1
    kw = dict(hot=hot, bias_amp=4.0 if hot else 0.1)
    T = sum(widths)
    recs = []
    if dec:
        for k in range(3):
            recs += dense("state%d" % (k + 1), S, widths[2 * k + 1], seed + 100 + 2 * k, 1.5)
    recs += dense(pre + "1", Lat if dec else 2 * NF, widths[0], seed, 3.0 if hot else 1.0)
    nin = widths[0]
    for l in range(2, 9):
        if l in (2, 4, 6):
            recs += gru(pre + str(l), nin, widths[l - 1], seed + 10 * l, **kw)
        else:
            recs += dense(pre + str(l), nin, widths[l - 1], seed + 10 * l, g)
        nin = widths[l - 1]
    if dec:
        recs += dense("dec_final", T, QFRAME, seed + 200, 2.0)
    else:
        recs += dense("bits_dense", ksize * T, Lat, seed + 200, 2.0)
        recs += dense("gdense1", T, gdense1, seed + 210, 2.0)
        recs += dense("gdense2", gdense1, S, seed + 220, 2.0)
    return recs


SMALL = (128, 64, 128, 64, 128, 64, 64, 64)
ODD = (128, 64, 192, 128, 64, 192, 24, 7)
WIDE = (512,) * 8
DENSE_BIASES = (["enc_dense%d_bias" % l for l in (1, 3, 5, 7, 8)] + ["bits_dense_bias", "gdense1_bias", "gdense2_bias"]
                + ["dec_dense%d_bias" % l for l in (1, 3, 5, 7, 8)] + ["state1_bias", "state2_bias", "state3_bias", "dec_final_bias"])


def _zeroed(blob: bytes, names) -> bytes:
    for nm in names:
        blob = replace_record(blob, nm, bytes(len(payload(blob, nm))))
    return blob


def _plc_zero_bias() -> bytes:
    return _zeroed(L.synthetic_model(1, L.VARIANT_INT8, plc_small=True), ["plc_dense1_bias", "plc_out_bias"])


def _rdo_k8() -> bytes:
    """the small synthetic encoder with an 8-tap conv (RDOVAE_KSIZE_MAX)"""
    blob = strip(L.synthetic_model(1, L.VARIANT_INT8, rdovae_small=True), set(DEC_NAMES))
    d = L.rdovae_dims(blob)["enc"]
    w = _sym(0x7108, 8 * d["T"] * d["L"], 2.0 * math.sqrt(3.0 / (8 * d["T"]))).astype(np.float32)
    return replace_record(blob, "bits_dense_weights", w.tobytes())


_BUILDERS = {
    # name: (kind, builder)
    "plc_uneven": ("plc", lambda: plc(64, 192, 320, 0x7001)),
    "plc_max": ("plc", lambda: plc(512, 512, 512, 0x7002)),
    "plc_hot": ("plc", lambda: plc(64, 128, 64, 0x7003, hot=True)),
    "plc_idx": ("plc", lambda: plc(64, 128, 64, 0x7004, idx=True)),
    "plc_subias_big": ("plc", lambda: plc(64, 128, 64, 0x7005, big=True)),
    "plc_zero_bias": ("plc", _plc_zero_bias),
    "rdo_k1": ("rdo", lambda: join(_base() + rdo_side(False, ODD, 3, 1, 0x7101, ksize=1, gdense1=5))),
    "rdo_k2": ("rdo", lambda: join(_base() + rdo_side(False, (128, 64, 128, 64, 128, 64, 64, 24), 33, 2, 0x7102,
                                                      ksize=2, gdense1=17))),
    "rdo_k8": ("rdo", _rdo_k8),
    "rdo_dec_odd": ("rdo", lambda: join(_base() + rdo_side(True, ODD, 1, 1, 0x7103))),
    "rdo_wide": ("rdo", lambda: join(_base() + rdo_side(False, WIDE, 16, 16, 0x7104, ksize=2, gdense1=16)
                                     + rdo_side(True, WIDE, 16, 16, 0x7105))),
    "rdo_hot": ("rdo", lambda: join(_base() + rdo_side(False, SMALL, 40, 32, 0x7106, ksize=4, gdense1=64, hot=True)
                                    + rdo_side(True, SMALL, 40, 32, 0x7107, hot=True))),
    "rdo_zero_bias": ("rdo", lambda: _zeroed(L.synthetic_model(1, L.VARIANT_INT8, rdovae_small=True), DENSE_BIASES)),
}
PLC_MODELS = [n for n, (k, _) in _BUILDERS.items() if k == "plc"]
RDO_MODELS = [n for n, (k, _) in _BUILDERS.items() if k == "rdo"]

# the dimensions every model is meant to have (tests/test_tile_cases_ref.py checks them against the host's parse)
PLC_DIMS = {"plc_uneven": (57, 64, 192, 320), "plc_max": (57, 512, 512, 512), "plc_hot": (57, 64, 128, 64),
            "plc_idx": (57, 64, 128, 64), "plc_subias_big": (57, 64, 128, 64), "plc_zero_bias": (57, 64, 128, 64)}


def _enc(widths, Lat, S, k, g1):
    return dict(L=Lat, S=S, T=sum(widths), kernel=k, widths=tuple(widths), gdense1=g1)


def _dec(widths, Lat, S):
    return dict(L=Lat, S=S, T=sum(widths), widths=tuple(widths))


RDO_DIMS = {
    "rdo_k1": {"enc": _enc(ODD, 3, 1, 1, 5), "dec": None},
    "rdo_k2": {"enc": _enc((128, 64, 128, 64, 128, 64, 64, 24), 33, 2, 2, 17), "dec": None},
    "rdo_k8": {"enc": _enc(SMALL, 40, 32, 8, 64), "dec": None},
    "rdo_dec_odd": {"enc": None, "dec": _dec(ODD, 1, 1)},
    "rdo_wide": {"enc": _enc(WIDE, 16, 16, 2, 16), "dec": _dec(WIDE, 16, 16)},
    "rdo_hot": {"enc": _enc(SMALL, 40, 32, 4, 64), "dec": _dec(SMALL, 40, 32)},
    "rdo_zero_bias": {"enc": _enc(SMALL, 40, 32, 4, 64), "dec": _dec(SMALL, 40, 32)},
}


@functools.lru_cache(maxsize=None)
def model(name: str) -> bytes:
    return _BUILDERS[name][1]()


class _Models(dict):
    """name -> blob, built on first use and kept"""

    def __missing__(self, name):
        if name not in _BUILDERS:
            raise KeyError(name)
        self[name] = model(name)
        return self[name]

    def names(self):
        return list(_BUILDERS)


MODELS = _Models()


def sides(name: str) -> list:
    """the entry points a model runs: "plc", "enc", "dec" """
    if name in PLC_DIMS:
        return ["plc"]
    return [s for s in ("enc", "dec") if RDO_DIMS[name][s] is not None]
