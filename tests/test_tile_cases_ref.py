"""The edge models of tests/tile_models.py and the cases of tests/tile_cases.py
on the CPU composition alone (no GPU): every model is one the host accepts
with the intended dimensions, every case reaches what it is there for, the
port's kernels agree with the reference's compiled ones on every (model, case),
and the committed digests are the composition's.  tests/test_gpu_tile_edge.py
compares the device with the same cached runs."""
import numpy as np
import pytest

import lpcnet_amd as L
import oracle_lib as O
import plc_ref as P
import tile_cases as T
import tile_models as M

SIDES = [(m, s) for m in M.MODELS.names() for s in M.sides(m)]
HOT = [("plc_hot", "plc"), ("rdo_hot", "enc"), ("rdo_hot", "dec")]


def values(r: dict) -> np.ndarray:
    """every output and snapshot float of a run"""
    parts = [a.ravel() for res in r["calls"] for a in res.values()] + [np.frombuffer(s, np.float32) for s in r["snaps"]]
    if r["init_snap"] is not None:
        parts.append(np.frombuffer(r["init_snap"], np.float32))
    return np.concatenate(parts)


def subnormal(v: np.ndarray) -> int:
    return int(np.sum((v != 0) & (np.abs(v) < T.TINY)))


@pytest.mark.parametrize("name", M.MODELS.names())
def test_model_loads_with_its_dimensions(name):
    blob = M.MODELS[name]
    L.validate_model(blob)
    if name in M.PLC_DIMS:
        assert L.plc_dims(blob) == M.PLC_DIMS[name]
    else:
        assert L.rdovae_dims(blob) == M.RDO_DIMS[name]
        for side in M.sides(name):  # a layer wider than 512 or an LDS need beyond 160 KiB would have been refused
            assert max(M.RDO_DIMS[name][side]["widths"]) <= 512


def test_edge_shapes_are_the_ones_meant():
    """unequal rounds over plc_gru's 8 waves (12 and 20 unit tiles), the
    largest width, every conv kernel size class, heads that are no multiple
    of 8 or 16"""
    assert [n // 16 % 8 for n in M.PLC_DIMS["plc_uneven"][2:]] == [4, 4]
    assert M.PLC_DIMS["plc_max"][1:] == (512, 512, 512)
    assert sorted(M.RDO_DIMS[m]["enc"]["kernel"] for m in ("rdo_k1", "rdo_k2", "rdo_k8", "rdo_hot")) == [1, 2, 4, 8]
    d = M.RDO_DIMS["rdo_k1"]["enc"]
    assert (d["T"], d["widths"][6:], d["gdense1"], d["L"], d["S"]) == (799, (24, 7), 5, 3, 1)
    # the encoder snapshots: GRU states and (ksize - 1) T floats of conv memory
    sizes = [4 * sum(T.dims_of(m, "enc")[1:3]) for m in ("rdo_k1", "rdo_k2", "rdo_k8")]
    assert sizes == [4 * 384, 4 * (192 + 664), 4 * (192 + 7 * 704)]


def _idx_rows(blob, name):
    w = P._arr(blob, P.records(blob), name + "_weights_idx", np.int32)
    rows, p = [], 0
    while p < len(w):
        rows.append([int(x) // 4 for x in w[p + 1:p + 1 + w[p]]])
        p += w[p] + 1
    return rows


def test_plc_idx_and_subias_big_are_what_they_claim():
    blob = M.MODELS["plc_idx"]
    for name, nin in (("plc_gru1", 64), ("plc_gru2", 128)):
        rows = _idx_rows(blob, name)
        assert any(len(r) == 0 for r in rows) and any(sorted(r) == list(range(nin // 4)) for r in rows)
        assert sum(len(set(r)) < len(r) for r in rows) == 2
    blob = M.MODELS["plc_subias_big"]
    for name in ("plc_gru1", "plc_gru2"):
        sub = P._arr(blob, P.records(blob), name + "_subias", np.float32).astype(np.float64) * (128.0 * 127.0)
        for half in np.split(sub, 2):  # beyond int32 on both sides, in both halves
            assert np.sum(half >= 2.0 ** 31) == 3 and np.sum(half < -2.0 ** 31) == 3


def test_ties_are_enumerated():
    """every k outside NO_TIE has a float x with fmaf(x, 127, 127) == k + .5
    (ties() asserts that exactly the k of NO_TIE have none); a run's two
    neighbours round to k + .5 -+ one ulp"""
    v, k = T.ties()
    assert set(k[k >= 0].tolist()) == set(range(254)) - T.NO_TIE
    q = (v.astype(np.float64) * 127.0 + 127.0).astype(np.float32)
    assert np.all(q[k >= 0] == k[k >= 0] + np.float32(.5))
    assert np.all(q[k < 0] != np.floor(q[k < 0]) + np.float32(.5))
    assert np.sum(k < 0) == 2 * len(set(k[k >= 0].tolist()))


@pytest.mark.parametrize("model,side", SIDES)
def test_finite_cases_hold_no_nan(model, side):
    """the condition of membership: a case not listed as non-finite holds no
    NaN in any output or snapshot of the reference"""
    for case in T.cases_of(model, side):
        if not T.nonfinite(side, case):
            assert not np.isnan(values(T.reference(model, side, case))).any(), case
    # and the control moves: outputs differ from call to call
    r = T.reference(model, side, "plain")
    f = T.FIELDS[side][0]
    assert not np.array_equal(r["calls"][0][f], r["calls"][-1][f])


@pytest.mark.parametrize("model,side", HOT)
def test_hot_models_saturate(model, side):
    """at least 5 % of the final states exactly +-1, quantised bytes 0 and 254,
    a z gate of exactly 0 and one of exactly 1, and states that still move"""
    r = T.reference(model, side, "plain")
    s, g = r["final_states"], r["gates"]
    assert np.mean(np.abs(s) == 1) >= 0.05, np.mean(np.abs(s) == 1)
    assert (s == 1).any() and (s == -1).any()
    assert g.bytes[0] > 0 and g.bytes[254] > 0
    assert g.z0 > 0 and g.z1 > 0
    assert np.mean(np.abs(s) < 0.9) >= 0.25


@pytest.mark.parametrize("model,side", SIDES)
def test_restored_states_reach_the_saturating_bytes(model, side):
    """st_over: v_cvt_pk_u8_f32's saturation at 255 and 0 (states in (1, 2] and
    [-2, -1)); st_ones: bytes 0 and 254"""
    g = T.reference(model, side, "st_over")["gates"]
    assert g.bytes[255] > 0 and g.bytes[0] > 0
    g = T.reference(model, side, "st_ones")["gates"]
    assert g.bytes[254] > 0 and g.bytes[0] > 0 and g.bytes[255] == 0


@pytest.mark.parametrize("case", ["sub", "tiny"])
def test_zero_bias_models_carry_subnormals(case):
    """Without dense biases a subnormal product survives the dense layer: with
    ``sub`` the encoder's conv memory (a saved dense1 output) and the decoder's
    states after dec_init hold subnormal, non-zero values, which the device
    must reproduce bit for bit (``tiny``: normal values below 1e-28 there).
    What a GRU reads is quantised (a subnormal is byte 127, as zero is) and
    every head sums GRU outputs, so no latent, qframe or PLC output can be
    subnormal; the PLC's subnormals end at plc_gru1's input, where the
    composition sees them."""
    bound = T.TINY if case == "sub" else np.float32(1e-28)
    small = lambda v: int(np.sum((v != 0) & (np.abs(v) < bound)))
    enc = T.reference("rdo_zero_bias", "enc", case)
    nt = T.dims_of("rdo_zero_bias", "enc")[1]
    assert small(np.frombuffer(enc["snaps"][-1], np.float32)[nt:]) > 0
    dec = T.reference("rdo_zero_bias", "dec", case)
    assert small(np.frombuffer(dec["init_snap"], np.float32)) > 0
    plc = T.reference("plc_zero_bias", "plc", case)
    if case == "sub":
        assert plc["gates"].sub_x > 0
    for r in (enc, dec, plc):
        assert subnormal(np.concatenate([a.ravel() for res in r["calls"] for a in res.values()])) == 0


@pytest.mark.parametrize("model", M.PLC_MODELS)
def test_plc_nan_input_ends_at_the_quantisation(model):
    """a NaN input is byte 0 at plc_dense1's quantisation: no output or state is NaN"""
    for case in ("nan_one", "nan_all", "fec_nan", "upd_nan"):
        r = T.reference(model, "plc", case)
        assert not np.isnan(values(r)).any(), case
        assert not np.array_equal(r["calls"][0]["out"], T.reference(model, "plc", "plain")["calls"][0]["out"]), case


@pytest.mark.parametrize("model", [m for m in M.RDO_MODELS if "enc" in M.sides(m)])
def test_encoder_nan_lives_as_long_as_the_conv_memory(model):
    """one NaN feature in call 1: NaN latents in exactly ksize consecutive calls, none after"""
    k = M.RDO_DIMS[model]["enc"]["kernel"]
    r = T.reference(model, "enc", "nan_one")
    assert [bool(np.isnan(c["latents"]).any()) for c in r["calls"]] == [True] * k + [False] * (len(r["calls"]) - k)
    if k > 1:  # mem_nan: the oldest tap leaves after one call
        m = T.reference(model, "enc", "mem_nan")
        assert [bool(np.isnan(c["latents"]).any()) for c in m["calls"]] == [False, True] + [False] * (len(m["calls"]) - 2)
        h = T.reference(model, "enc", "mem_huge")
        assert [bool(np.isnan(c["latents"]).any()) for c in h["calls"][1:k]] == [True] * (k - 1)


@pytest.mark.parametrize("model,side", SIDES)
def test_nan_states_persist(model, side):
    r = T.reference(model, side, "st_nan")
    assert np.isnan(r["final_states"]).any()
    f = T.FIELDS[side][0]
    assert np.isnan(r["calls"][-1][f]).any()


def test_ties_tell_the_roundings_apart():
    """over every model's st_ties state: round-half-even and floor(v + .5)
    differ on at least 100 state elements, and a separate multiply and add
    differs from the fused one on some"""
    differ = unfused = 0
    for model, side in SIDES:
        nt = T.dims_of(model, side)[1]
        x = np.frombuffer(T.reference(model, side, "st_ties")["restore"][1], np.float32)[:nt]
        v = (x.astype(np.float64) * 127.0 + 127.0).astype(np.float32)  # the fused form, rounded once
        differ += int(np.sum(np.rint(v) != np.floor(v + np.float32(.5))))
        unfused += int(np.sum(np.rint(x * np.float32(127) + np.float32(127)) != np.rint(v)))
    assert differ >= 100 and unfused > 0, (differ, unfused)


def test_both_row_forms_on_every_dense_kind():
    """Over all models, the FMA form (rows % 16 == 0) and the generic one both
    occur on every dense layer kind that can take either: dense7, dense8 on both
    sides, bits_dense, gdense1, gdense2.  dense1 / 3 / 5 and state1..3 feed a
    GRU (a multiple of 64 rows) and dec_final has 80 rows: FMA only."""
    forms = set()
    for model, side in SIDES:
        forms |= T.reference(model, side, "plain")["forms"]
    for kind in ("enc_dense7", "enc_dense8", "dec_dense7", "dec_dense8", "bits_dense", "gdense1", "gdense2"):
        assert {(kind, "fma"), (kind, "generic")} <= forms, kind
    for kind in ("enc_dense1", "enc_dense3", "enc_dense5", "dec_dense1", "state1", "state2", "state3", "dec_final"):
        assert (kind, "fma") in forms and (kind, "generic") not in forms


def test_the_comparison_rule():
    """same: NaN where the reference is NaN (either quiet pattern), the same
    bits elsewhere (-0.0 is not 0.0), and no NaN at all in a finite case"""
    ref = np.array([1.0, np.nan, -0.0, 1e-42], np.float32)
    x86 = ref.view(np.uint32).copy()
    x86[1] = 0xFFC00000
    assert T.same(ref, ref, True) and T.same(x86.view(np.float32), ref, True)
    assert not T.same(ref, ref, False)  # a NaN in a case not listed as non-finite
    for i, v in ((0, np.float32(1.0000001)), (1, np.float32(0)), (2, np.float32(0.0)), (3, np.float32(0))):
        dev = ref.copy()
        dev[i] = v
        assert not T.same(dev, ref, True), i
        assert "case call 3 out" in T.diff("model", "case", 3, "out", dev, ref) and "[%d]" % i in T.diff("model", "case", 3, "out", dev, ref)
    sig = ref.view(np.uint32).copy()
    sig[1] = 0x7F800001  # a signalling NaN is not what either machine makes
    assert not T.same(sig.view(np.float32), ref, True)
    assert T.canon(x86.view(np.float32)) == T.canon(ref)


def _agree(model, side, table):
    bad = []
    for case in T.cases_of(model, side):
        a, b = T.reference(model, side, case), T.reference(model, side, case, table)
        nf = T.nonfinite(side, case)
        for c, (ra, rb) in enumerate(zip(a["calls"], b["calls"])):
            for f in T.FIELDS[side]:
                if not T.same(ra[f], rb[f], nf):
                    bad.append(T.diff(model, case, c + 1, f, ra[f], rb[f], " (port against %s)" % table))
            if not T.same(a["snaps"][c], b["snaps"][c], nf):
                bad.append(T.diff(model, case, c + 1, "snapshot", a["snaps"][c], b["snaps"][c], " (port against %s)" % table))
        if a["init_snap"] is not None and not T.same(a["init_snap"], b["init_snap"], nf):
            bad.append(T.diff(model, case, "init", "snapshot", a["init_snap"], b["init_snap"]))
    return bad


@pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref (the reference's compiled kernels) not built")
@pytest.mark.parametrize("model,side", SIDES)
def test_port_and_reference_tables_agree(model, side):
    """Every (model, case) under ``same``: the reference's compiled matrix
    kernels under the port's activations on any host, and the reference's own
    activations too where this CPU's rcpps is the pinned Intel table (as
    tests/test_plc_model.py)."""
    bad = _agree(model, side, "hybrid")
    tab, wrong = O.ref_rcp_table()
    if wrong == 0 and np.array_equal(tab, O.RCP_TABLE):
        bad += _agree(model, side, "ref")
    assert not bad, "\n".join(bad[:10])


def test_fixture_digests():
    fix = T.fixture()
    assert sorted(fix) == sorted(T.key(*r) for r in T.RUNS)
    bad = [T.key(*r) for r in T.RUNS if T.reference_digest(*r) != fix[T.key(*r)]]
    assert not bad, bad
