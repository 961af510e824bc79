"""The edge-case fixture of the conditioning network
(tests/golden/cond_edge.npz, sequences and models of tests/cond_frames.py):
what the CPU oracle's run_frame_network answers on it -- with the port
kernels, with the AVX2 build of the same restatement and, where oracle/_ref
is built, with the reference's own compiled kernels -- and the facts the
GPU tests rely on: the finite class is finite, the NaN counts of the
non-finite class, the separation of the wrong pitch forms, the support of
the impulse.

PARITY OF THE GLUE UNPINNED by a reference build: run_frame_network itself
(lpcnet.c:82-120) includes lpcnet_private.h -> the generated nnet_data.h,
which is absent, so it cannot be compiled from the reference.  What runs here
is oracle/lpcnet_oracle.c's restatement of those lines over the reference's
compiled sgemv_accum16, vec_tanh and lpc_from_cepstrum (oracle/_ref) or their
ports; the pitch expression of that restatement is pinned by pitch_forms
(see test_pitch_forms_are_separated)."""
import numpy as np
import pytest

import cond_frames as CF
import lpcnet_amd as L
import oracle_lib as O

needs_ref = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref (the reference's compiled kernels) not built")
needs_avx2 = pytest.mark.skipif(not O.have_avx2_build(), reason="the AVX2 build of the oracle is absent")
FX = CF.fixture()
R, S = len(CF.RUNS), len(CF.NAMES)


def live(model_name: str, seq: str, **kw) -> np.ndarray:
    """records [12, WORDS] of the live oracle on the fixture's features"""
    variant, constants, _ = CF.MODELS[model_name]
    o = O.Oracle(CF.model(model_name), variant, constants=constants, **kw)
    out = []
    for f in CF.features_of(seq):
        o.synthesize(f, 0)
        out.append(CF.oracle_record(o))
    return np.stack(out)


def check_model(model_name: str, **kw):
    errors = []
    for seq in CF.MODELS[model_name][2]:
        rec = live(model_name, seq, **kw)
        for f in range(CF.NFRAMES):
            errors += CF.fixture_diff(model_name, seq, f, rec[f])
    assert not errors, "%d mismatches; the first: %s" % (len(errors), "\n".join(errors[:6]))


# -- fixture facts ---------------------------------------------------------------

def test_fixture_shapes():
    assert list(FX["names"]) == CF.NAMES and len(set(CF.NAMES)) == S and list(FX["models"]) == list(CF.MODELS)
    assert [(str(FX["models"][m]), str(FX["names"][s])) for m, s in FX["runs"]] == CF.RUNS
    assert FX["features"].shape == (S, CF.NFRAMES, CF.NF) and FX["features"].dtype == np.float32
    assert FX["digests"].shape == (R, CF.NFRAMES, 32) and FX["digests"].dtype == np.uint8
    assert FX["gru_b_cond"].shape == (R, CF.NFRAMES, 48) and FX["lpc"].shape == (R, CF.NFRAMES, 16)
    assert FX["nan_count"].shape == FX["finite"].shape == (R, CF.NFRAMES)
    assert FX["last"].shape == (R, CF.WORDS) and FX["last"].dtype == np.uint32
    assert CF.NFRAMES == 12 and CF.WORDS == 1152 + 48 + 16 + 168 + 256 + 1
    for r in range(R):
        # the last digest is that of the stored record; the stored fields are its own
        assert CF.digest(FX["last"][r]) == FX["digests"][r, -1].tobytes(), CF.RUNS[r]
        assert np.array_equal(CF.field(FX["last"][r], "lpc"), FX["lpc"][r, -1]), CF.RUNS[r]
        assert np.array_equal(CF.canon(FX["last"][r]), FX["last"][r]), CF.RUNS[r]


def test_sequences_are_what_their_names_say():
    f = {n: CF.features_of(n) for n in CF.NAMES}
    base = f["const"][0]
    sub = lambda x: (np.abs(x) < 2.0 ** -126) & (x != 0)  # noqa: E731
    assert not f["zeros"].view(np.uint32).any() and (f["neg_zeros"].view(np.uint32) == 0x80000000).all()
    assert (f["const"] == base).all() and 0 < base[0] < 4 and np.abs(base).max() < 4
    assert np.array_equal(f["impulse"][4], base) and not np.delete(f["impulse"], 4, 0).any()
    assert np.array_equal(f["alt_sign"][0::2], f["const"][0::2]) and np.array_equal(f["alt_sign"][1::2], -f["const"][1::2])
    assert (f["loud"][:, 0] == 40).all() and np.array_equal(f["loud"][:, 1:18], f["const"][:, 1:18] * np.float32(10))
    assert sub(f["subnormal"]).sum() >= 12 * 15 and not sub(f["tiny"]).any() and np.abs(f["tiny"]).max() < 1e-29
    assert sorted(set(f["corr_edges"][:, 19].tolist())) == [-10.0, -0.5, 0.5, 10.0]
    assert np.abs(f["lpc_wide"][:, :18]).max() > 16
    mags = np.abs(f["scale_ramp"][:, 0]) / abs(base[0])
    assert mags[0] < 2e-6 and mags[-1] > 5e4 and np.abs(f["scale_lo"]).max() <= np.abs(base).max()
    assert np.isnan(f["nan_band"][5, 3]) and np.isnan(f["nan_band"]).sum() == 1
    assert f["inf_c0"][4, 0] == np.inf and f["inf_c0"][8, 0] == -np.inf
    assert f["inf_pitch"][3, 18] == np.inf and f["inf_pitch"][6, 18] == -np.inf and np.isnan(f["inf_pitch"][9, 18])
    assert (f["lpc_overflow"][3:6, 0] == 200).all() and f["max_float"][5, 7] == np.float32(3e38)
    assert set(f["pitch_huge"][:, 18].tolist()) == {1e10, -1e10}
    for n in CF.FINITE:
        assert np.isfinite(f[n]).all(), n
    for n in CF.NAMES:
        if n.startswith("pitch_"):  # base cepstrum and correlation, only f18 moves
            assert np.array_equal(np.delete(f[n], 18, 1), np.delete(f["const"], 18, 1)), n


def test_pitch_edges_reach_both_clamps_and_every_boundary():
    v = np.concatenate([CF.features_of("pitch_edges%d" % k)[:, 18] for k in range(4)])
    assert np.array_equal(v.view(np.uint32), CF.pitch_edge_values().view(np.uint32))
    rows = [CF.pitch_ref(x) for x in v]
    raw = [int(np.floor((0.1 + float(np.float32(50) * x)) + 100.0)) for x in v]
    # below, at and above each clamp; both rows at every listed boundary
    assert min(raw) < 33 <= min(rows) and max(raw) > 255 >= max(rows)
    for k in (33, 34, 100, 176, 254, 255, 256):
        assert {k - 1, k} <= set(raw), k
    for k in (34, 100, 176, 255):
        lo, hi = CF._floor_boundary(k)
        assert CF.pitch_ref(lo) == k - 1 and CF.pitch_ref(hi) == k and np.nextafter(lo, np.float32(np.inf)) == hi
        assert lo in v and hi in v
    assert set(rows) == {33, 34, 99, 100, 175, 176, 253, 254, 255}


def test_pitch_forms_are_separated():
    """Each wrong form of the pitch expression picks another embedding row
    than the reference at two values or more, one at least inside the
    decoder's range; on pitch_only another row is another conditioning
    vector, so the fixture pins the reference's form (a mutation of the
    oracle's pitch line to any of the four fails test_port_kernels on
    pitch_forms)."""
    v = CF.features_of("pitch_forms")[:, 18]
    assert np.array_equal(v.view(np.uint32), CF.pitch_form_values().view(np.uint32))
    sep = CF.form_separation(v)
    assert set(sep) == {"all_float", "all_double", "no_tenth", "rint"}
    for form, vals in sep.items():
        assert len(set(vals)) >= 2, form
        assert any(CF.DECODER_RANGE[0] <= x <= CF.DECODER_RANGE[1] for x in vals), form
    # another row is another record: constant sequences of the two rows differ on pitch_only
    o = [O.Oracle(CF.model("pitch_only"), 0) for _ in range(2)]
    x = CF.features_of("const")[0].copy()
    for form, fn in CF.WRONG_FORMS.items():
        f18 = np.float32(sep[form][0])
        rows = (CF.pitch_ref(f18), fn(f18))
        assert rows[0] != rows[1]
        recs = []
        for k in range(2):
            o[k].reset()
            x[18] = np.float32((rows[k] - 100) / 50.0)
            assert CF.pitch_ref(x[18]) == rows[k]
            for _ in range(3):  # past the two silent FEATURES_DELAY frames
                o[k].synthesize(x, 0)
            recs.append(CF.oracle_record(o[k]))
        assert (CF.field(recs[0], "gru_a_cond") != CF.field(recs[1], "gru_a_cond")).sum() > 1000, form


def test_generators_reproduce_the_fixture_features():
    """The maker's input is reproducible: RandomState is a frozen stream."""
    import sys
    sys.path.insert(0, CF.GOLDEN.rsplit("/", 1)[0])
    import make_cond_golden as M
    for k, n in enumerate(CF.NAMES):
        got = CF.make(n, M.lpc_finite)
        assert got.dtype == np.float32 and got.shape == (CF.NFRAMES, CF.NF), n
        assert np.array_equal(got.view(np.uint32), FX["features"][k].view(np.uint32)), n


def test_variant_models():
    plain = CF.model("int8")
    for name in CF.VARIANTS:
        blob = CF.model(name)
        L.validate_model(blob)
        assert len(blob) == len(plain) and blob != plain
    recs = {n: CF.records(CF.model(n)) for n in ("int8", "pitch_only", "zero_bias")}
    for (n0, _, p0), (_, _, p1), (_, _, p2) in zip(recs["int8"], recs["pitch_only"], recs["zero_bias"]):
        assert (p0 != p1) == (n0 == "feature_conv1_weights"), n0
        assert p0 == p2 or n0 in CF.BIASES, n0
        if n0 in CF.BIASES:
            assert not any(p2), n0
    w = CF._floats(CF.find(recs["pitch_only"], "feature_conv1_weights")).reshape(CF.CONV_K, CF.FIN, CF.COND)
    assert not w[:, :CF.NF].any() and np.count_nonzero(w[:, CF.NF:]) > w[:, CF.NF:].size // 2
    fo = CF.records(CF.model("features_only"))
    for (n0, _, p0), (_, _, p3) in zip(recs["zero_bias"], fo):
        assert (p0 != p3) == (n0 == "feature_conv1_weights"), n0
    w = CF._floats(CF.find(fo, "feature_conv1_weights")).reshape(CF.CONV_K, CF.FIN, CF.COND)
    assert not w[:, CF.NF:].any() and np.count_nonzero(w[:, :CF.NF]) > w[:, :CF.NF].size // 2


# -- classes -----------------------------------------------------------------------

def test_finite_class_is_finite():
    for r, (m, s) in enumerate(CF.RUNS):
        if s in CF.FINITE:
            assert FX["finite"][r].all() and not FX["nan_count"][r].any(), (m, s)
            assert np.isfinite(FX["last"][r, :-1].view(np.float32)).all(), (m, s)
    # pitch_huge is finite where it matters: on pitch_only
    assert FX["finite"][CF.run_of("pitch_only", "pitch_huge")].all()


def test_nonfinite_class_nan_counts():
    """The NaN counts the GPU tests assert: non-zero where the sequence makes
    NaN, never "everything" where something finite must survive."""
    nc = lambda m, s: FX["nan_count"][CF.run_of(m, s)].tolist()  # noqa: E731
    assert nc("int8", "nan_band") == [0, 0, 0, 0, 0, 1329, 1457, 1472, 1328, 1200, 0, 0]
    assert nc("int8", "lpc_overflow") == [0, 0, 0, 0, 0, 16, 16, 16, 0, 0, 0, 0]       # LPC of frames 3..5, two frames late
    assert nc("g092_d3", "lpc_overflow") == [0, 0, 0, 0, 0, 0, 16, 16, 16, 0, 0, 0]    # three frames late
    assert nc("e2e_g09_d1", "lpc_overflow") == [0] * 12                                # rc2lpc: no cepstrum involved
    assert nc("int8", "scale_ramp") == [0] * 10 + [16, 16]
    for m in ("int8", "fp32", "g092_d3", "e2e_g09_d1"):
        for s in CF.NONFINITE:
            c = np.array(nc(m, s))
            assert c.max() < CF.WORDS - 1 and (c.any() or (m, s[:4]) in (("e2e_g09_d1", "lpc_"), ("e2e_g09_d1", "scal"))), (m, s)
        assert nc(m, "nan_band")[10:] == [0, 0] and nc(m, "max_float")[10:] == [0, 0]   # the NaN leaves the conv memories
    for r, (m, s) in enumerate(CF.RUNS):
        assert np.array_equal(FX["nan_count"][r] == 0, FX["finite"][r]) or s in ("inf_c0", "inf_pitch", "max_float", "pitch_huge"), (m, s)


def test_impulse_support():
    """One non-zero frame changes frames 4..8 and nothing else: before it and
    from frame 9 on every record equals the zeros sequence's, bit for bit."""
    for m in ("int8", "fp32", "g092_d3", "e2e_g09_d1"):
        di, dz = FX["digests"][CF.run_of(m, "impulse")], FX["digests"][CF.run_of(m, "zeros")]
        same = [di[f].tobytes() == dz[f].tobytes() for f in range(CF.NFRAMES)]
        assert same == [f < 4 or f >= 9 for f in range(CF.NFRAMES)], (m, same)
        a, z = live(m, "impulse"), live(m, "zeros")
        for f in range(CF.NFRAMES):
            d = CF.diff("impulse", f, a[f], z[f], "zeros sequence")
            assert bool(d) == (4 <= f <= 8), (m, f, d)
            ga = CF.field(a[f], "gru_a_cond") != CF.field(z[f], "gru_a_cond")
            c1 = CF.field(a[f], "conv1_mem") != CF.field(z[f], "conv1_mem")
            assert ga.any() == (4 <= f <= 8) and c1.any() == (4 <= f <= 5), (m, f)


def test_subnormals_survive_on_features_only():
    """Without biases and without the pitch embedding the subnormal products
    reach the outputs; with the generator's biases they are swallowed (the
    subnormal sequence's conditioning then equals the zeros sequence's)."""
    sub = lambda w: ((np.abs(w) < 2.0 ** -126) & (w != 0)).sum()  # noqa: E731
    last = FX["last"][CF.run_of("features_only", "subnormal")][:-1].view(np.float32)
    assert sub(CF.field(last, "gru_a_cond")) > 500 and sub(CF.field(last, "conv2_mem")) > 100, \
        (sub(CF.field(last, "gru_a_cond")), sub(CF.field(last, "conv2_mem")))
    assert not FX["last"][CF.run_of("features_only", "zeros")][:1200].any()
    tiny = FX["last"][CF.run_of("features_only", "tiny")][:-1].view(np.float32)
    assert np.count_nonzero(CF.field(tiny, "gru_a_cond")) > 1000 and np.abs(CF.field(tiny, "gru_a_cond")).max() < 1e-25
    assert np.array_equal(CF.field(FX["last"][CF.run_of("int8", "subnormal")], "gru_a_cond"),
                          CF.field(FX["last"][CF.run_of("int8", "zeros")], "gru_a_cond"))


# -- the oracle reproduces the fixture ------------------------------------------------

@pytest.mark.parametrize("model_name", list(CF.MODELS))
def test_port_kernels(model_name):
    check_model(model_name)


@needs_avx2
@pytest.mark.parametrize("model_name", list(CF.MODELS))
def test_avx2_build(model_name):
    check_model(model_name, avx2_build=True)


@needs_ref
@pytest.mark.parametrize("model_name", list(CF.MODELS))
def test_reference_kernels(model_name):
    check_model(model_name, kernels=O.ref_kernels())


def test_diff_names_field_and_indices():
    rec = FX["last"][CF.run_of("int8", "const")].copy()
    other = rec.copy()
    other[1152 + 5] ^= 1
    other[-1] += 1
    d = CF.diff("const", 11, other, rec)
    assert len(d) == 2 and "const frame 11: gru_b_cond" in d[0] and "[5]" in d[0] and "frame_count" in d[1]
    x = rec.copy()
    x[3] = 0xFFC00000
    assert CF.canon(x)[3] == CF.NAN and CF.nan_count(CF.canon(x)) == 1
