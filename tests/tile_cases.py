"""Edge-case call sequences for the PLC predictor and the RDO-VAE, their CPU
reference runs and the comparison rule.  TEST INFRASTRUCTURE ONLY.

A case is a deterministic sequence of calls on ONE stream of one model of
tests/tile_models.py, through one entry point ("plc": compute_plc_pred, "enc":
dred_rdovae_encode_dframe, "dec": dec_init_states + decode_qframe): the input
of every call and, for the state cases, a snapshot restored before the second
call.  ``reference`` runs a case once on the CPU composition (plc_ref /
rdovae_ref, on the port's or the reference's compiled kernels) and keeps every
call's outputs and the snapshot after every call; the GPU tests lay the cases
over the streams of a batch and compare each stream with its case's solo run
under ``same``: NaN where the reference is NaN, the same bits elsewhere.

Calls are counted from 1 in the case descriptions (call 1 is the first).
"""
from __future__ import annotations

import functools
import hashlib
import json
import os

import numpy as np

import lpcnet_amd as L
import oracle_lib as O
import plc_ref as P
import rdovae_ref as R
import tile_models as M

NF = L.NB_FEATURES
NAN = 0x7FC00000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tile_edge.json")
F = np.float32
TINY = np.finfo(np.float32).tiny

INPUTS = ["plain", "zeros", "neg_zeros", "sub", "tiny", "loud", "huge", "max_float", "nan_one", "inf_pos", "inf_neg", "nan_all"]
PLC_ONLY = ["fec_nan", "upd_nan"]
DEC_ONLY = ["lat_big", "init_big"]
STATES = ["st_ties", "st_ones", "st_over", "st_small", "st_nan"]
ENC_ONLY = ["mem_nan", "mem_huge"]
# the cases whose reference run may hold NaN; every other case must be NaN-free (tests/test_tile_cases_ref.py)
NONFINITE = {"nan_one", "inf_pos", "inf_neg", "nan_all", "init_big", "fec_nan", "upd_nan", "st_nan", "mem_nan", "mem_huge"}
# the RDO-VAE's dense1 has no bound on its sum: at 1e9 and 3e38 tanh8_approx's X^4 is inf and inf * rcp(inf) is NaN
RDO_NONFINITE = NONFINITE | {"huge", "max_float"}


def nonfinite(side: str, case: str) -> bool:
    return case in (NONFINITE if side == "plc" else RDO_NONFINITE)


FIELDS = {"plc": ("out",), "enc": ("latents", "state"), "dec": ("qframe",)}


def cases_of(model: str, side: str) -> list:
    """the cases that run on a model's entry point"""
    c = INPUTS + {"plc": PLC_ONLY, "dec": DEC_ONLY, "enc": []}[side] + STATES
    if side == "enc" and M.RDO_DIMS[model]["enc"]["kernel"] > 1:  # ksize 1: no conv memory
        c = c + ENC_ONLY
    return c


RUNS = [(m, s, c) for m in M.MODELS.names() for s in M.sides(m) for c in cases_of(m, s)]


def ncalls(model: str, side: str) -> int:
    if side == "plc":
        return 6
    if side == "dec":
        return R.NDEC
    k = M.RDO_DIMS[model]["enc"]["kernel"]
    return 6 if k <= 4 else k + 2


def dims_of(model: str, side: str):
    """(input floats per call, GRU state floats, conv memory floats, decoder S)"""
    if side == "plc":
        d = M.PLC_DIMS[model]
        return P.PLC_IN, d[2] + d[3], 0, 0
    d = M.RDO_DIMS[model][side]
    nt = sum(d["widths"][1:6:2])
    if side == "enc":
        return 2 * NF, nt, (d["kernel"] - 1) * d["T"], 0
    return d["L"], nt, 0, d["S"]


# ---- rounding ties of the state quantisation -----------------------------------
def _q(x) -> np.float32:
    """fmaf(x, 127, 127): the double product and sum of a float and 127 are exact"""
    return F(np.float64(x) * 127.0 + 127.0)


# k for which no float x has fmaf(x, 127, 127) == k + .5: near x = -1 the floats
# lie 2^-24 apart, 127 x + 127 moves in steps of 127 * 2^-24, coarser than the
# ulp of k + .5, and is exact or rounds elsewhere
NO_TIE = set(range(0, 15)) | set(range(18, 30)) | set(range(36, 44)) | set(range(52, 59))


@functools.lru_cache(maxsize=None)
def ties():
    """(values, k): every float x with fmaf(x, 127, 127) == k + .5 exactly, k
    = 0..253, each run of them followed by its two float neighbours (the
    floats just below and just above the run); k[i] is the tie's k, -1 for a
    neighbour.  A k outside NO_TIE has at least one tie."""
    vals, ks, without = [], [], set()
    down, up = F(-3), F(3)
    for k in range(254):
        v = F(k + .5)
        x = F((k - 126.5) / 127.0)
        cand = [x]
        a = b = x
        for _ in range(6):
            a, b = np.nextafter(a, down), np.nextafter(b, up)
            cand += [a, b]
        hit = [c for c in cand if _q(c) == v]
        if not hit:
            without.add(k)
            continue
        lo = hi = hit[0]
        while _q(np.nextafter(lo, down)) == v:
            lo = np.nextafter(lo, down)
        while _q(np.nextafter(hi, up)) == v:
            hi = np.nextafter(hi, up)
        run = [lo]
        while run[-1] != hi:
            run.append(np.nextafter(run[-1], up))
        vals += run + [np.nextafter(lo, down), np.nextafter(hi, up)]
        ks += [k] * len(run) + [-1, -1]
    assert without == NO_TIE, sorted(without ^ NO_TIE)
    vals, ks = np.array(vals, np.float32), np.array(ks)
    assert np.all(np.abs(vals) < 1.01)
    vals.setflags(write=False)
    return vals, ks


OVER = np.array([1 + 2.0 ** -23, -(1 + 2.0 ** -23), 2, -2, 1.25, -1.25, 1.5, -1.5, 2 - 2.0 ** -22, -(2 - 2.0 ** -22),
                 1 + 1 / 254., -(1 + 1 / 254.), 1 + 1.5 / 127, -(1 + 1.5 / 127), 1.75, -1.001], np.float32)
SMALL = np.array([-0.0, 1e-42, -1e-42, 1e-30, -1e-30], np.float32)
# just outside gru_state_plausible's [-2, 2]
REFUSED = [np.nextafter(F(2), F(3)), np.nextafter(F(-2), F(-3)), F(np.inf), F(-np.inf)]


def state_pattern(case: str, n: int, saved: np.ndarray, offset: int = 0) -> np.ndarray:
    """the n GRU state floats a state case restores; ``saved`` is the state the
    reference held (st_nan keeps it but for every 7th element)"""
    i = np.arange(n)
    if case == "st_ties":
        v = ties()[0]
        return v[(offset + 977 * i) % len(v)].copy()  # 977 is prime: a short state still spans every k
    if case == "st_ones":
        return np.where(i % 2 == 0, F(1), F(-1)).astype(np.float32)
    if case == "st_over":
        return OVER[(i + offset) % len(OVER)].copy()
    if case == "st_small":
        return SMALL[(i + offset) % len(SMALL)].copy()
    if case == "st_nan":
        v = saved.copy()
        v[::7] = np.nan
        return v
    raise KeyError(case)


def restored(model: str, side: str, case: str, snap: bytes) -> bytes | None:
    """the snapshot a state case restores before call 2, from the one the
    reference saved after call 1"""
    if case not in STATES + ENC_ONLY:
        return None
    _, nt, nmem, _ = dims_of(model, side)
    v = np.frombuffer(snap, np.float32).copy()
    assert v.size == nt + nmem
    off = 191 * M.MODELS.names().index(model) + (97 if side == "dec" else 0)
    if case in STATES:
        v[:nt] = state_pattern(case, nt, v[:nt], off)
    elif case == "mem_nan":
        v[nt:nt + M.RDO_DIMS[model]["enc"]["T"]] = np.nan  # the oldest tap only
    else:  # mem_huge
        v[nt:] = np.array([3e38, -3e38, np.inf, -np.inf], np.float32)[np.arange(nmem) % 4]
    return v.tobytes()


# ---- inputs ----------------------------------------------------------------------
def _edit(case: str, x: np.ndarray, scale_only: bool = False) -> np.ndarray:
    """the input case applied to the plain inputs x [calls, dim]"""
    x = x.copy()
    dim = x.shape[1]
    with np.errstate(all="ignore"):
        if case == "zeros":
            x[:] = 0
        elif case == "neg_zeros":
            x[:] = -0.0
        elif case == "sub":
            x[:] = 1e-42
        elif case == "tiny":
            x *= F(1e-30)
        elif case == "loud":
            x *= F(1e4)
        elif case == "huge":
            x[:] = 1e9
        elif scale_only:
            pass
        elif case == "max_float":
            x[:, 7 % dim] = 3e38
        elif case == "nan_one":
            x[0, 5 % dim] = np.nan
        elif case == "inf_pos":
            x[0, 3 % dim] = np.inf
        elif case == "inf_neg":
            x[0, 3 % dim] = -np.inf
        elif case == "nan_all":
            x[0] = np.nan
    return x


@functools.lru_cache(maxsize=None)
def inputs(model: str, side: str, case: str):
    """(x [calls, dim], the decoder's initial state [S] or None), read-only"""
    n = ncalls(model, side)
    dim, _, _, S = dims_of(model, side)
    init = None
    if side == "plc":
        x = np.stack([np.zeros(dim, np.float32) if v is None else v for v in P.call_inputs(0, n)])
        x = _edit(case, x)
        if case in PLC_ONLY:  # everything NaN but the flag, in calls 1 and 4
            for c in (0, 3):
                x[c] = np.nan
                x[c, dim - 1] = -1 if case == "fec_nan" else 1
    elif side == "enc":
        x = _edit(case, R.enc_inputs(0, n))
    else:
        x = _edit(case, R.dec_latents(0, dim, n))
        init = _edit(case, R.dec_state(0, S)[None], scale_only=True)[0]
        if case == "lat_big":
            x[:] = np.where(np.arange(dim) % 2 == 0, F(30), F(-30))
        if case == "init_big":
            init = np.where(np.arange(S) % 2 == 0, F(1e6), F(-1e6)).astype(np.float32)
            init[S // 2] = np.nan
        init.setflags(write=False)
    x.setflags(write=False)
    return x, init


# ---- the reference run -------------------------------------------------------------
def _table(table: str):
    """"port", "ref" (the reference's compiled kernels, oracle/_ref) or
    "hybrid" (the reference's matrix kernels under the port's activations:
    everything that does not pass through the host CPU's rcpps)"""
    if table == "hybrid":
        from test_plc_model import _Hybrid
        return _Hybrid()
    return O.kernel_table(O.ref_kernels() if table == "ref" else O.port_kernels())


class Gates:
    """what the GRUs of a run saw (the hook of plc_ref.PlcRef._gru)"""

    def __init__(self):
        self.z0 = self.z1 = self.sub_x = 0
        self.bytes = np.zeros(256, np.int64)

    def __call__(self, g, x, state, z, r, h):
        self.z0 += int(np.sum(z == 0))
        self.z1 += int(np.sum(z == 1))
        self.sub_x += int(np.sum((x != 0) & (np.abs(x) < TINY)))  # subnormal, non-zero GRU inputs
        for v in (x, state):
            self.bytes += np.bincount(O.quantize_u8(v), minlength=256)


@functools.lru_cache(maxsize=None)
def reference(model: str, side: str, case: str, table: str = "port", skip: frozenset = frozenset()) -> dict:
    """One solo run, computed once and left unchanged: {"calls": [{field:
    array}], "snaps": [snapshot after every call], "restore": {call index:
    snapshot restored before it}, "init_snap": the decoder's snapshot after
    dec_init, "gates": Gates, "forms": the dense row forms taken}.  The calls
    (from 0) in ``skip`` are left out, as for a stream that is inactive in
    them: their entry in "calls" is None and the snapshot stays."""
    blob, k = M.MODELS[model], _table(table)
    x, init = inputs(model, side, case)
    ref = {"plc": P.PlcRef, "enc": R.RdoEnc, "dec": R.RdoDec}[side](blob, k)
    ref.gru_hook = gates = Gates()
    out = dict(calls=[], snaps=[], restore={}, init_snap=None, gates=gates)
    with np.errstate(all="ignore"):
        if side == "dec":
            ref.init(init)
            out["init_snap"] = ref.save()
        for c in range(len(x)):
            if c == 1:
                st = restored(model, side, case, out["snaps"][0])
                if st is not None:
                    ref.restore(st)
                    out["restore"][1] = st
            if c in skip:
                out["calls"].append(None)
                out["snaps"].append(ref.save())
                continue
            if side == "plc":
                res = dict(out=ref.predict(x[c]))
            elif side == "enc":
                z, s = ref.encode(x[c])
                res = dict(latents=z, state=s)
            else:
                res = dict(qframe=ref.qframe(x[c]))
            for v in res.values():
                v.setflags(write=False)
            out["calls"].append(res)
            out["snaps"].append(ref.save())
    out["forms"] = frozenset(getattr(ref, "forms", ()))
    out["final_states"] = np.frombuffer(out["snaps"][-1], np.float32)[:dims_of(model, side)[1]]
    return out


# ---- comparison ----------------------------------------------------------------------
def bits(a) -> np.ndarray:
    if isinstance(a, (bytes, bytearray)):
        return np.frombuffer(a, np.uint32)
    return np.ascontiguousarray(a, np.float32).view(np.uint32).ravel()


def _quiet_nan(w: np.ndarray) -> np.ndarray:
    return ((w & np.uint32(0x7FC00000)) == np.uint32(0x7FC00000))


def same(dev, ref, nonfinite: bool) -> bool:
    """The rule of cond_frames: where the reference is NaN the device must be
    a quiet NaN (x86 makes 0xFFC00000, the GPU 0x7FC00000; either counts),
    everywhere else the uint32 views are equal.  A reference with a NaN in a
    case not listed as non-finite never compares equal."""
    d, r = bits(dev), bits(ref)
    if d.shape != r.shape:
        return False
    nan = np.isnan(r.view(np.float32))
    if nan.any() and not nonfinite:
        return False
    return bool(np.all(_quiet_nan(d[nan])) and np.array_equal(d[~nan], r[~nan]))


def diff(model: str, case: str, call, field: str, dev, ref, where: str = "") -> str:
    """names model, case, call, field and the first differing indices"""
    d, r = bits(dev), bits(ref)
    if d.shape != r.shape:
        return "%s/%s call %s %s%s: %d words, expected %d" % (model, case, call, field, where, d.size, r.size)
    nan = np.isnan(r.view(np.float32))
    bad = np.flatnonzero(np.where(nan, ~_quiet_nan(d), d != r))
    if not bad.size:
        return "%s/%s call %s %s%s: the reference holds %d NaN in a finite case" % (model, case, call, field, where, nan.sum())
    i = bad[0]
    return ("%s/%s call %s %s%s differs at %d of %d indices, first %s: got %r (0x%08x), expected %r (0x%08x)"
            % (model, case, call, field, where, bad.size, d.size, bad[:8].tolist(), float(d[i:i + 1].view(np.float32)[0]), d[i],
               float(r[i:i + 1].view(np.float32)[0]), r[i]))


def canon(a) -> bytes:
    w = bits(a).copy()
    w[np.isnan(w.view(np.float32))] = NAN
    return w.tobytes()


def digest(side: str, calls: list, snaps: list, init_snap=None) -> str:
    """sha256 (its first 80 bits, as hex) over every call's outputs and snapshot, NaNs as 0x7FC00000"""
    h = hashlib.sha256()
    if init_snap is not None:
        h.update(canon(init_snap))
    for res, snap in zip(calls, snaps):
        for f in FIELDS[side]:
            h.update(canon(res[f]))
        h.update(canon(snap))
    return h.hexdigest()[:20]


def key(model: str, side: str, case: str) -> str:
    return "%s/%s/%s" % (model, side, case)


def reference_digest(model: str, side: str, case: str, table: str = "port") -> str:
    r = reference(model, side, case, table)
    return digest(side, r["calls"], r["snaps"], r["init_snap"])


@functools.lru_cache(maxsize=None)
def fixture() -> dict:
    with open(GOLDEN) as f:
        return json.load(f)
