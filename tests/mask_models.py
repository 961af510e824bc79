"""Synthetic models with a chosen sparsity mask.  TEST INFRASTRUCTURE ONLY.

The GRU_A recurrent product is the one part of synthesis whose device code
depends on the model's mask: mf_plan.cpp turns the blob's block index into
register tables, per-wave group counts and merge rows, and the kernels
dispatch on those counts.  ``build(rows)`` makes a model whose GRU_A mask is
exactly ``rows``; ``FAMILIES`` names the masks the tests run (hand-made edge
cases of the planner and the kernels' dispatch, and Sparsify-like masks of
other generator seeds); ``build_gru_b(kind)`` does the same for the GRU_B
input matrix, which the matrix-core kernels read as a dense tile built from
the index.

Everything is drawn from the generator below (splitmix64 of a counter:
integer arithmetic only, the same numbers with any numpy), never numpy's.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import lpcnet_amd as L
from test_ingest import find, idx_words, join, put_idx, records, set_size

NA, NB = 384, 16
NUB = NA // 8   # unit blocks (8-row block rows) per gate
NCB = NA // 4   # column blocks
_M = (1 << 64) - 1


def _mix(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & _M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M
    return z ^ (z >> 31)


class Rng:
    """splitmix64, one value at a time (the masks)."""

    def __init__(self, seed: int):
        self.s = _mix(seed)

    def next(self) -> int:
        self.s = (self.s + 0x9E3779B97F4A7C15) & _M
        return _mix(self.s)

    def below(self, n: int) -> int:
        return ((self.next() >> 32) * n) >> 32

    def sample(self, n: int, k: int = NCB) -> list:
        """n of the column blocks 0..k-1 without repetition, ascending."""
        pool = list(range(k))
        for i in range(n):
            j = i + self.below(k - i)
            pool[i], pool[j] = pool[j], pool[i]
        return sorted(pool[:n])


def uniform(seed: int, n: int) -> np.ndarray:
    """n doubles in [0, 1) with 24 random bits each: splitmix64 of the
    counters seed' + 1 .. seed' + n, vectorised (uint64 arithmetic wraps)."""
    with np.errstate(over="ignore"):
        z = np.uint64(_mix(seed)) + np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float64) / float(1 << 24)


def draw_blocks(seed: int, amps: np.ndarray):
    """One 8x4 block per entry of ``amps``, uniform in +-amp, each adjacent
    pair clipped to |a| + |b| <= 0.992 before quantisation as model_gen.cpp's
    make_sparse does (non-saturating: 255 (q0 + q1) stays inside int16).
    Returns (w float64 [n, 8, 4], q int8 [n, 8, 4])."""
    n = len(amps)
    w = (2.0 * uniform(seed, 32 * n) - 1.0).reshape(n, 8, 2, 2) * np.asarray(amps, np.float64).reshape(n, 1, 1, 1)
    s = np.abs(w).sum(-1, keepdims=True)
    w = np.where(s > 0.992, w * (0.992 / np.maximum(s, 1e-30)), w).reshape(n, 8, 4)
    q = np.clip(np.rint(128.0 * w), -128, 127).astype(np.int8)
    return w, q


def _put(rec, payload: bytes):
    block = (len(payload) + 63) // 64 * 64
    rec[2] = bytearray(payload) + bytearray(block - len(payload))
    set_size(rec, len(payload), block)


def _floats(rec) -> np.ndarray:
    return idx_words(rec).view(np.float32)


def _pack(w, q, variant: int) -> bytes:
    """int8 blocks are w[r*4+c]; fp32 blocks are w[c*8+r] (emit_sparse)."""
    if variant == L.VARIANT_INT8:
        return q.tobytes()
    return np.ascontiguousarray(w.transpose(0, 2, 1), np.float32).tobytes()


def build(rows, variant: int = 0, seed: int = 0) -> bytes:
    """L.synthetic_model(1, variant) with the GRU_A recurrent mask ``rows``:
    144 lists of column blocks 0..95, gate-major (z, r, h x 48 unit blocks),
    duplicates allowed.  Weights uniform in +-0.6 sqrt(min(1, 19 / len(row)))
    (the generator's 0.6 at its h density of 19 blocks a row, scaled down on
    longer rows so that the gates' sums keep their spread)."""
    assert len(rows) == 3 * NUB and all(0 <= cb < NCB for r in rows for cb in r)
    recs = records(L.synthetic_model(1, variant))
    idx, amps = [], []
    for r in rows:
        idx.append(len(r))
        idx.extend(4 * cb for cb in r)
        amps.extend([0.6 * math.sqrt(min(1.0, 19.0 / max(1, len(r))))] * len(r))
    w, q = draw_blocks(0x6A00 + seed, np.array(amps, np.float64))
    colsum = np.zeros(3 * NA)
    k = 0
    for rb, r in enumerate(rows):
        colsum[8 * rb:8 * rb + 8] = q[k:k + len(r)].astype(np.int64).sum((0, 2)) / 128.0
        k += len(r)
    bias = _floats(find(recs, "sparse_gru_a_bias"))
    sub = bias.copy()
    sub[3 * NA:] = (bias[3 * NA:].astype(np.float64) - colsum).astype(np.float32)  # model_gen.cpp: bias - sum(q) / 128
    _put(find(recs, "sparse_gru_a_recurrent_weights"), _pack(w, q, variant))
    put_idx(find(recs, "sparse_gru_a_recurrent_weights_idx"), idx)
    _put(find(recs, "sparse_gru_a_subias"), sub.tobytes())
    return join(recs)


def gru_a_rows(blob: bytes) -> list:
    """the GRU_A mask of a blob, as ``build`` takes it"""
    w = idx_words(find(records(blob), "sparse_gru_a_recurrent_weights_idx"))
    rows, p = [], 0
    while p < len(w):
        rows.append([int(x) // 4 for x in w[p + 1:p + 1 + w[p]]])
        p += w[p] + 1
    return rows


def _gates(z, r, h):
    return [list(x) for x in z] + [list(x) for x in r] + [list(x) for x in h]


def _families() -> dict:
    g = Rng(1)
    rnd = g.sample
    E = [[] for _ in range(NUB)]
    U = range(NUB)
    full = list(range(NCB))
    bank = lambda k: [8 * j + k for j in range(12)]  # 12 column blocks of one LDS bank class (cb % 8)
    F = {}
    # waves with no group at all in a gate: one block in z (row 0, last column), one in h (last row, column 0)
    F["one_block"] = _gates([[NCB - 1]] + E[1:], E, E[:-1] + [[0]])
    # own 0 with hosted groups: z empty, four r rows of 48
    F["z_empty_r_long"] = _gates(E, [rnd(48) if u < 4 else [] for u in U], [rnd(19) for _ in U])
    # one full row, every other z row empty
    F["z_one_full"] = _gates([full] + E[1:], [rnd(5) for _ in U], [rnd(19) for _ in U])
    # hosted pieces in h only (first and last row full), r empty
    F["h_only_long"] = _gates([rnd(2) for _ in U], E, [full if u in (0, NUB - 1) else rnd(8) for u in U])
    # 17 unit blocks with pieces: one more than the wide split form's part area holds
    F["units17_long"] = _gates([rnd(20) if u < 17 else rnd(3) for u in U], [rnd(4) for _ in U], [rnd(19) for _ in U])
    # exactly its 16, in z and in h
    F["units16_long"] = _gates([rnd(20) if u < 16 else rnd(3) for u in U], [rnd(4) for _ in U],
                               [rnd(40) if u >= 32 else rnd(10) for u in U])
    # every row exactly at the register caps: the largest unsplit tables
    F["at_caps"] = _gates([rnd(16) for _ in U], [rnd(16) for _ in U], [rnd(32) for _ in U])
    # every block of a row in one bank class: the matcher's "any free slot" fallback
    F["same_bank"] = _gates([bank(0) for _ in U], [bank(1) for _ in U], [bank(u % 2) + bank(2) for u in U])
    F["same_bank_long"] = _gates([bank(0) for _ in U], [bank(0) for _ in U],
                                 [bank(0) + bank(1) + bank(2) if u < 6 else bank(0) for u in U])
    # one position twenty times: the duplicates spread over own and hosted pieces
    F["dup_in_long"] = _gates([[3] * 20 if u == 5 else rnd(4) for u in U], [rnd(4) for _ in U], [rnd(19) for _ in U])
    # one block over the caps on too many rows for any split: the lockstep kernel, long rows
    F["cap_edges"] = _gates([rnd(16) if u % 2 else rnd(17) for u in U], [rnd(16) for _ in U],
                            [rnd(32) if u % 3 else rnd(33) for u in U])
    F["all17"] = _gates([rnd(17) for _ in U], [rnd(17) for _ in U], [rnd(33) for _ in U])
    # fully dense: 13,824 blocks, 442 KB of int8 GRU_A weights
    F["dense"] = _gates([full] * NUB, [full] * NUB, [full] * NUB)
    # Sparsify-like masks of other generator seeds: seed 2 has a wide split form, 3 and 5 have none
    for seed in SKEWED_SEEDS:
        F["skewed_seed%d" % seed] = gru_a_rows(L.synthetic_model(seed, 0, skewed=True))
    return F


SKEWED_SEEDS = (2, 3, 5)
FAMILIES = _families()


def wide_split_exists(rows) -> bool:
    """mfw_kernel's split form (mf_plan.cpp mfw_split_tables) exists exactly
    when every gate's blocks beyond the register caps (16 / 16 / 32) make at
    most 16 pieces of at most a cap each, over at most 16 unit blocks."""
    for g, cap in enumerate((16, 16, 32)):
        beyond = [max(0, len(r) - cap) for r in rows[g * NUB:(g + 1) * NUB]]
        if sum((b + cap - 1) // cap for b in beyond) > 16 or sum(b > 0 for b in beyond) > 16:
            return False
    return True


@functools.lru_cache(maxsize=None)
def model(name: str, variant: int = 0) -> bytes:
    """the blob of a family (cached: about 5 MB each)"""
    return build(FAMILIES[name], variant, sorted(FAMILIES).index(name))


GRU_B_KINDS = ("every_second_block", "one_row_block_empty")


@functools.lru_cache(maxsize=None)
def build_gru_b(kind: str, variant: int = 0) -> bytes:
    """L.synthetic_model(1, variant) with a GRU_B input mask: every second
    column block of each row block (alternating phase), or row block 2 empty.
    The kept blocks keep their weights; the first half of gru_b_subias is
    recomputed as emit_sparse does (bias - sum(q) / 128)."""
    assert kind in GRU_B_KINDS
    recs = records(L.synthetic_model(1, variant))
    wrec, irec = find(recs, "gru_b_weights"), find(recs, "gru_b_weights_idx")
    per = 32 if variant == L.VARIANT_INT8 else 128
    old = []  # the generator's mask: per row block, its blocks' input offsets
    w, p = idx_words(irec), 0
    while p < len(w):
        old.append([int(x) for x in w[p + 1:p + 1 + w[p]]])
        p += w[p] + 1
    assert len(old) == 3 * NB // 8
    size = np.frombuffer(bytes(wrec[1][12:16]), np.int32)[0]
    blocks = np.frombuffer(bytes(wrec[2][:size]), np.uint8).reshape(-1, per)
    idx, keep, colsum, k = [], [], np.zeros(3 * NB), 0
    for rb, pos in enumerate(old):
        kept = [t for t in range(len(pos))
                if (kind == "every_second_block" and t % 2 == rb % 2) or (kind == "one_row_block_empty" and rb != 2)]
        idx.append(len(kept))
        idx.extend(pos[t] for t in kept)
        for t in kept:
            b = blocks[k + t]
            if variant == L.VARIANT_INT8:
                q = b.view(np.int8).astype(np.float64).reshape(8, 4)
            else:  # q8: roundf(128 w), clipped; the block is w[c*8+r]
                x = 128.0 * b.view(np.float32).astype(np.float64).reshape(4, 8).T
                q = np.clip(np.trunc(x + np.copysign(0.5, x)), -128, 127)
            colsum[8 * rb:8 * rb + 8] += q.sum(1) / 128.0
            keep.append(k + t)
        k += len(pos)
    bias = _floats(find(recs, "gru_b_bias"))
    sub = _floats(find(recs, "gru_b_subias")).copy()
    sub[:3 * NB] = (bias[:3 * NB].astype(np.float64) - colsum).astype(np.float32)
    _put(wrec, blocks[keep].tobytes())
    put_idx(irec, idx)
    _put(find(recs, "gru_b_subias"), sub.tobytes())
    return join(recs)
