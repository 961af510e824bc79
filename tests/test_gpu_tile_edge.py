"""The PLC predictor (plc_kernel.hip) and the RDO-VAE encoder and decoder
(rdovae_kernel.hip), which share plc_gru of gru_tile.h, on the edge models of
tests/tile_models.py and the cases of tests/tile_cases.py: shapes with unequal
rounds per wave and the largest widths, conv kernels of 1, 2 and 8 taps, heads
of 1 to 33 rows, saturating gates, restored states on rounding ties, beyond
+-1, subnormal and NaN, non-finite inputs and conv memory, index rows that are
empty, full or list a block twice, and subias seeds beyond int32.

A case is one stream's sequence of calls; its reference is the solo CPU run
of tile_cases.reference, computed once.  A batch lays a model's cases over its
streams (layout): 33 streams (two full 16-stream tiles and a third of one
stream) in order, the same batch in reversed order -- every case at other
slots, in another 4-stream dense group, beside other neighbours, the NaN and
saturated cases next to the finite ones -- and 5 streams (a partial tile) with
the cases rotated by two.  Every stream's outputs of every call and its saved
state after every call are compared under tile_cases.same (NaN where the
reference is NaN, the same bits elsewhere), and the digest of the device's data
must be the committed one of tests/golden/tile_edge.json.  A mismatch names
model, case, slot, call, field and the first indices."""
import numpy as np
import pytest

import lpcnet_amd as L
import oracle_lib as O
import tile_cases as T
import tile_models as M

pytestmark = pytest.mark.gpu

NF = L.NB_FEATURES
FILL = np.float32(-77.25)
SIDES = [(m, s) for m in M.MODELS.names() for s in M.sides(m)]
COUNTS = {}  # model/side -> (case, slot) comparisons made


@pytest.fixture(scope="module", autouse=True)
def report_counts():
    yield
    for k in sorted(COUNTS):
        print("\ntile edge comparisons %s: %d" % (k, COUNTS[k]), end="")
    print()


def layout(cases: list, B: int, how: str) -> list:
    """the case of every slot: the cases cyclically, in order, reversed, or rotated by two"""
    n = len(cases)
    if how == "reversed":
        return [cases[(B - 1 - i) % n] for i in range(B)]
    return [cases[(i + (2 if how == "rotated" else 0)) % n] for i in range(B)]


def third_odd(s: int, call: int) -> bool:
    """the active mask of the mask tests: every third stream is inactive on odd calls"""
    return not (s % 3 == 2 and call % 2 == 1)


class Side:
    """one entry point of a batch: restore, call, save"""

    def __init__(self, b, model, side):
        self.b, self.model, self.side = b, model, side
        self.which = {"plc": 0, "enc": 1, "dec": 2}[side]
        d = T.dims_of(model, side)
        self.dim, self.S = d[0], d[3]
        if side == "enc":
            e = M.RDO_DIMS[model]["enc"]
            self.outs = {"latents": e["L"], "state": e["S"]}
        else:
            self.outs = {"out": NF} if side == "plc" else {"qframe": 4 * NF}

    def reset(self):
        if self.side == "plc":
            self.b.plc_reset()
        else:
            self.b.rdovae_reset(None, self.which)

    def save(self, s):
        return self.b.plc_save_state(s) if self.side == "plc" else self.b.rdovae_save_state(s, self.which)

    def restore(self, s, st):
        if self.side == "plc":
            self.b.plc_restore_state(s, st)
        else:
            self.b.rdovae_restore_state(s, st, self.which)

    def call(self, x, active):
        """{field: [B, n]} with the rows of inactive streams left at FILL"""
        out = {f: np.full((self.b.B, n), FILL) for f, n in self.outs.items()}
        if self.side == "plc":
            self.b.plc_predict(x, active=active, out=out["out"])
        elif self.side == "enc":
            self.b.rdovae_encode(x, active=active, latents=out["latents"], state=out["state"])
        else:
            self.b.rdovae_decode_qframe(x, active=active, out=out["qframe"])
        return out


def run(b, model: str, side: str, slots: list, mask=None, table: str = "port") -> list:
    """One batch through its slots' cases.  Returns the mismatches (diff
    lines); checks outputs, snapshots and, without a mask, the digests."""
    B, io = len(slots), Side(b, model, side)
    assert B == b.B
    n = T.ncalls(model, side)
    skips = [frozenset(c for c in range(n) if mask and not mask(s, c)) for s in range(B)]
    refs = [T.reference(model, side, slots[s], table, skips[s]) for s in range(B)]
    xs = [T.inputs(model, side, c) for c in slots]
    bad, dev = [], [dict(calls=[], snaps=[], init_snap=None) for _ in range(B)]
    io.reset()

    def check(s, call, field, got, exp):
        if not T.same(got, exp, T.nonfinite(side, slots[s])):
            bad.append(T.diff(model, slots[s], call, field, got, exp, " (slot %d of %d)" % (s, B)))

    if side == "dec":
        b.rdovae_dec_init(np.stack([x[1] for x in xs]))
        for s in range(B):
            dev[s]["init_snap"] = io.save(s)
            check(s, "init", "snapshot", dev[s]["init_snap"], refs[s]["init_snap"])
    for c in range(n):
        if c == 1:
            for s in range(B):
                if 1 in refs[s]["restore"]:
                    io.restore(s, refs[s]["restore"][1])
        active = np.array([c not in skips[s] for s in range(B)])
        before = [io.save(s) for s in range(B)] if mask else None
        out = io.call(np.stack([x[0][c] for x in xs]), active if mask else None)
        for s in range(B):
            snap = io.save(s)
            if active[s]:
                res = {f: out[f][s] for f in out}
                for f in out:
                    check(s, c + 1, f, res[f], refs[s]["calls"][c][f])
            else:  # untouched: the output rows, and the state bit for bit
                res = None
                assert all(np.all(out[f][s] == FILL) for f in out), (model, slots[s], s, c)
                assert snap == before[s], (model, slots[s], s, c)
            check(s, c + 1, "snapshot", snap, refs[s]["snaps"][c])
            dev[s]["calls"].append(res)
            dev[s]["snaps"].append(snap)
    if not mask and table == "port":
        fix = T.fixture()
        for s in range(B):
            if T.digest(side, dev[s]["calls"], dev[s]["snaps"], dev[s]["init_snap"]) != fix[T.key(model, side, slots[s])]:
                bad.append("%s/%s (slot %d of %d): the digest of the device's data is not the fixture's" % (model, slots[s], s, B))
    COUNTS[model + "/" + side] = COUNTS.get(model + "/" + side, 0) + B
    return bad


@pytest.mark.parametrize("model,side", SIDES)
def test_cases_over_the_slots(require_gpu, model, side):
    cases = T.cases_of(model, side)
    blob = M.MODELS[model]
    bad = []
    b = L.LPCNetBatch(33, 0, blob)
    if side == "plc":
        assert b.plc_info() == M.PLC_DIMS[model]
    else:
        assert b.rdovae_info() == M.RDO_DIMS[model]
    for how in ("in order", "reversed"):
        bad += run(b, model, side, layout(cases, 33, how))
    b.close()
    b = L.LPCNetBatch(5, 0, blob)
    bad += run(b, model, side, layout(cases, 5, "rotated"))
    b.close()
    assert not bad, "%d mismatches:\n%s" % (len(bad), "\n".join(bad[:12]))


@pytest.mark.parametrize("model", [m for m in M.RDO_MODELS if "dec" in M.sides(m)])
def test_decode_all_is_the_qframe_path(require_gpu, model):
    """decode_all as one launch over a case's initial state and latents: equal
    to the solo reference's qframes (and so to the qframe path of
    test_cases_over_the_slots), the persistent decoder state untouched bit
    for bit, NaN states included."""
    cases = [c for c in T.cases_of(model, "dec") if c not in T.STATES]  # a packet has no restore in its middle
    slots = layout(cases, 33, "reversed")
    B, n = len(slots), T.ncalls(model, "dec")
    b = L.LPCNetBatch(B, 0, M.MODELS[model])
    io = Side(b, model, "dec")
    # a persistent state that is not the reset one: NaN in every 7th element of every second stream
    b.rdovae_dec_init(np.stack([T.inputs(model, "dec", "plain")[1]] * B))
    b.rdovae_decode_qframe(np.stack([T.inputs(model, "dec", "plain")[0][0]] * B))
    for s in range(0, B, 2):
        io.restore(s, T.reference(model, "dec", "st_nan")["restore"][1])
    before = [io.save(s) for s in range(B)]
    xs = [T.inputs(model, "dec", c) for c in slots]
    f = np.full((B, 4 * n, NF), FILL)
    b.rdovae_decode_all(np.stack([x[1] for x in xs]), np.stack([x[0] for x in xs]), out=f)
    bad = []
    for s in range(B):
        exp = np.concatenate([r["qframe"] for r in T.reference(model, "dec", slots[s])["calls"]])
        if not T.same(f[s], exp, T.nonfinite("dec", slots[s])):
            bad.append(T.diff(model, slots[s], "1..%d" % n, "decode_all", f[s], exp, " (slot %d of %d)" % (s, B)))
    assert [io.save(s) for s in range(B)] == before
    b.close()
    COUNTS[model + "/dec"] = COUNTS.get(model + "/dec", 0) + B
    assert not bad, "%d mismatches:\n%s" % (len(bad), "\n".join(bad[:12]))


@pytest.mark.parametrize("model,side", [("plc_hot", "plc"), ("rdo_hot", "enc"), ("rdo_k2", "enc"), ("rdo_hot", "dec")])
def test_active_mask(require_gpu, model, side):
    """Every third stream is inactive on odd calls: its state, conv memory and
    output rows are untouched, next to NaN and saturated neighbours too; the
    active streams equal a reference that skipped the same calls."""
    b = L.LPCNetBatch(33, 0, M.MODELS[model])
    bad = run(b, model, side, layout(T.cases_of(model, side), 33, "in order"), mask=third_odd)
    b.close()
    assert not bad, "%d mismatches:\n%s" % (len(bad), "\n".join(bad[:12]))


@pytest.mark.parametrize("model,side", [("plc_hot", "plc"), ("rdo_hot", "enc"), ("rdo_hot", "dec")])
def test_snapshot_just_outside_the_bound_is_refused(require_gpu, model, side):
    """2 + ulp, -2 - ulp and +-inf in a GRU state: refused with the reason, the
    state unchanged; +-2 themselves and NaN are accepted (st_over, st_nan)."""
    b = L.LPCNetBatch(3, 0, M.MODELS[model])
    io = Side(b, model, side)
    r = T.reference(model, side, "plain")
    nt = T.dims_of(model, side)[1]
    for s in range(3):
        io.restore(s, r["snaps"][0])
    for k, v in enumerate(T.REFUSED):
        st = np.frombuffer(r["snaps"][1], np.float32).copy()
        st[(37 * k + 5) % nt] = v
        with pytest.raises(L.LPCNetError) as e:
            io.restore(1, st.tobytes())
        assert "GRU state outside [-2, 2]: not a state this engine produced" in str(e.value), v
        assert [io.save(s) for s in range(3)] == [r["snaps"][0]] * 3, v
    b.close()


@pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref (the reference's compiled kernels) not built")
@pytest.mark.parametrize("model,side", [("plc_hot", "plc"), ("rdo_hot", "enc"), ("rdo_hot", "dec")])
def test_table_form_matches_live_reference(require_gpu, model, side):
    """With this host's rcpps table the kernels run their table form (or, on
    the pinned Intel table, the hardware-reciprocal form) and equal the
    composition on the reference's compiled kernels, live on this CPU: the hot
    models, every case, the non-finite ones among them."""
    tab, wrong = L.host_rcp_table()
    assert wrong == 0, "this host's rcpps is not a 12-bit exponent-invariant table"
    cases = T.cases_of(model, side)
    b = L.LPCNetBatch(len(cases), 0, M.MODELS[model])
    b.set_rcp_table(tab)
    intel = np.array_equal(tab[::2], L.rcp_table()) and np.array_equal(tab[1::2], L.rcp_table())
    assert b.info().rcp_hw == (1 if intel else 0)
    print("\ntile edge table form: rcp_hw = %d" % b.info().rcp_hw)
    bad = run(b, model, side, cases, table="ref")
    b.set_rcp_table(None)
    b.close()
    assert not bad, "%d mismatches:\n%s" % (len(bad), "\n".join(bad[:12]))
