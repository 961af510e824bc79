"""The concealment machine's edge cases (tests/conceal_edge.py) on the CPU:
the committed fixture tests/golden/conceal_edge.npz against its recomputation
through tests/conceal_ref.py and tests/conceal_nc_ref.py, and that every case
goes where it was sent, read from the counters those two keep beside their
arithmetic.  The recomputation needs the reference's compiled kernels
(oracle/_ref) and is skipped without them, as in tests/test_conceal_ref.py;
the rest reads the fixture alone."""
import functools
import os

import numpy as np
import pytest

import conceal_edge as CE
import conceal_ref as CR
import enc_ref

needs_ref = pytest.mark.skipif(not enc_ref.have_ref(), reason="oracle/_ref (the reference's compiled kernels) not built")
RUN_IDS = [r[0] for r in CE.RUNS]
LARGEST_FIXTURE = 838881  # tests/golden/enc_packets.npz


@functools.lru_cache(maxsize=None)
def computed(run):
    """(arrays, counters per stream) of a run, computed once for the tests that read them."""
    out, counts = CE.compute_run(run)
    for v in out.values():
        v.setflags(write=False)
    return out, counts


def test_fixture_shape():
    fx = CE.fixture()
    assert os.path.getsize(CE.GOLDEN) <= LARGEST_FIXTURE
    assert np.array_equal(fx["lost"], CE.lost_matrix()) and fx["lost"][CE.BURST, 3:23].all()
    assert fx["edge_pcm"].shape == (5, CR.NTICKS, 160) and fx["edge_pcm"].dtype == np.int16
    assert fx["f_rows"].shape == (len(CE.F_CASES), CE.NROWS, 20) and fx["f_rows"].dtype == np.float32
    for run, options, delay in CE.RUNS:
        S = CE.nstreams(run)
        assert S <= 10
        assert fx[f"{run}_pcm"].shape == (S, CR.NTICKS, 160) and fx[f"{run}_pcm"].dtype == np.int16
        assert fx[f"{run}_buf"].shape == (S, CR.plc_buf_size(delay) + 160) and fx[f"{run}_buf"].dtype == np.int16
        assert fx[f"{run}_ctrl"].shape == (S, len(CR.CTRL)) and fx[f"{run}_dc"].dtype == np.float64
        if run.startswith("f_"):
            assert fx[f"{run}_gru_a"].shape == (S, 384) and fx[f"{run}_enc"].dtype == np.uint8
        else:
            assert fx[f"{run}_digests"].shape == (S, len(CE.BIG), 32)
            assert np.isfinite(fx[f"{run}_features"]).all()
        if not options & CR.DC_FILTER:
            assert not fx[f"{run}_dc"].any()


def test_inputs_are_the_generators():
    fx = CE.fixture()
    for k, v in CE.compute_inputs().items():
        assert v.dtype == fx[k].dtype and np.array_equal(v.view(np.uint8), fx[k].view(np.uint8)), k


def test_edge_signals_and_rows_are_what_they_say():
    fx = CE.fixture()
    pcm = dict(zip(CE.EDGE_SIGNALS, fx["edge_pcm"].astype(np.int32)))
    assert pcm["dc_hi_tone"].max() > 32400 and pcm["dc_hi_tone"].min() > 27000 and abs(pcm["dc_hi_tone"].mean() - 30000) < 50
    assert pcm["dc_lo_tone"].max() < -28000 and pcm["dc_lo_tone"].min() >= -32768 and abs(pcm["dc_lo_tone"].mean() + 30500) < 50
    assert set(np.unique(pcm["square_fs"])) == {-32768, 32767} and np.array_equal(pcm["square_fs"][0, :80], pcm["square_fs"][5, 80:])
    assert pcm["fullnoise"].min() < -32700 and pcm["fullnoise"].max() > 32700
    assert pcm["dc_step"][:CE.STEP_FRAME].min() > 16000 and pcm["dc_step"][CE.STEP_FRAME:].max() < -16000
    rows = dict(zip([n for n, _ in CE.F_CASES], fx["f_rows"]))
    finite = [n for n in rows if n not in ("nan_row", "nan_c0", "inf_row")]
    assert all(np.isfinite(rows[n]).all() for n in finite)
    assert np.isnan(rows["nan_row"][:, :18]).sum() == 1 and np.isfinite(rows["nan_row"][:, 18:]).all()
    assert np.isnan(rows["nan_c0"][:, 0]).sum() == 1 and np.isnan(rows["nan_c0"]).sum() == 1
    assert sorted(rows["inf_row"][np.isinf(rows["inf_row"])]) == [-np.inf, np.inf] and np.isinf(rows["inf_row"][:, 0]).sum() == 2
    assert not np.isnan(rows["inf_row"]).any()
    assert np.abs(rows["extremes"]).max() >= 40 and np.abs(rows["huge_finite"]).max() >= 1e10
    z = rows["zeros_subnormals"]
    tiny = np.finfo(np.float32).tiny
    assert (np.signbit(z) & (z == 0)).any() and ((z != 0) & (np.abs(z) < tiny)).any()
    # features[18] on both sides of the pitch index clamp (lpcnet.c:98-100: rows 33 .. 255)
    f18 = rows["pitch_clamps"][:, 18]
    assert (f18 < (33 - 100.1) / 50).any() and (f18 > (255 - 100.1) / 50 + .02).any()
    assert f18.min() <= -5 and f18.max() >= 10


@needs_ref
@pytest.mark.parametrize("run", RUN_IDS)
def test_fixture_equals_recomputation(run):
    fx = CE.fixture()
    out, _ = computed(run)
    for k, v in out.items():
        want = fx[f"{run}_{k}"]
        assert v.dtype == want.dtype and v.shape == want.shape, k
        assert np.array_equal(v.view(np.uint8), want.view(np.uint8)), (run, k)


def test_packing_keeps_every_sample():
    fx = CE.fixture()
    packed = CE.pack({k: v for k, v in fx.items()})
    assert packed["d_pcm"].shape == (6, CR.NTICKS, len(CE.RUNS_D), 160) and packed["e_pcm"].shape == (10, CR.NTICKS, len(CE.RUNS_E), 160)
    again = CE.unpack(packed)
    assert sorted(again) == sorted(fx) and all(again[k].tobytes() == fx[k].tobytes() for k in fx)


# -- the aims ------------------------------------------------------------------------------------------

@needs_ref
@pytest.mark.parametrize("run,options,delay", CE.RUNS_D, ids=[r[0] for r in CE.RUNS_D])
def test_delay_runs_reach_their_aims(run, options, delay):
    _, counts = computed(run)
    buf = CR.plc_buf_size(delay)
    assert all(c["move_max"] == max(buf, 160) for c in counts)  # CM_SHIFT moves PLC_BUF_SIZE shorts on every path
    if delay >= 3:
        assert buf > 512, "the move's third register carries data"
    lossy = range(1, 6)
    if options & 3 == CR.CAUSAL:
        assert all(counts[s]["restore_at_delay"] > 0 for s in lossy), "PLC_RESTORE reads the ring's last copy"
    else:
        assert not any(c["restore_at_delay"] for c in counts)  # the codec mode restores copy FEATURES_DELAY - 1
    assert counts[4]["loss_ge_10"] == 3
    if options & CR.DC_FILTER:  # fullnoise alone drives the filter here; set E is there for the rest
        assert counts[5]["dc_remove_wrap"] > 0 and counts[5]["dc_add_wrap"] > 0 and counts[5]["l_negative"] > 0
    else:
        assert not any(c[k] for c in counts for k in ("dc_remove_wrap", "dc_add_wrap", "l_negative", "delta_trunc"))


# what each edge signal is there for, on either script, in every run of set E
SIGNAL_AIMS = {"dc_hi_tone": ("dc_add_wrap",), "dc_lo_tone": ("l_negative", "dc_add_wrap"), "square_fs": ("dc_remove_wrap", "dc_add_wrap"),
               "fullnoise": ("dc_remove_wrap", "dc_add_wrap", "l_negative"), "dc_step": ("dc_remove_wrap", "dc_add_wrap", "l_negative")}
# runs in which some stream has a negative delta that (int) and floor tell apart; e_causal_dc_2 has none
DELTA_TRUNC_RUNS = ("e_causal_dc_4", "e_codec_dc_0", "e_noncausal_dc_0")


@needs_ref
@pytest.mark.parametrize("run,options,delay", CE.RUNS_E, ids=[r[0] for r in CE.RUNS_E])
def test_edge_pcm_runs_reach_their_aims(run, options, delay):
    fx = CE.fixture()
    _, counts = computed(run)
    nc = options & 3 == CR.NONCAUSAL
    for s, (sig, script) in enumerate(CE.E_CASES):
        c, name = counts[s], CE.EDGE_SIGNALS[sig]
        for aim in SIGNAL_AIMS[name]:
            assert c[aim] > 0, (run, name, script, aim)
        if script == CE.BURST:
            # 20 lost ticks: loss_count 10 .. 20 (the non-causal mode attenuates before it counts: 10 .. 19)
            assert c["loss_ge_10"] == (10 if nc else 11) and c["clamp"] > 0, (run, name)
        else:
            assert c["loss_ge_10"] == 0
        if not nc:
            assert c["move_max"] == max(CR.plc_buf_size(delay), 160)
            assert (c["restore_at_delay"] > 0) == (options & 3 == CR.CAUSAL)
    # dc_mem at both ends of int16 and, after the step, across zero with syn_dc live
    dc = fx[f"{run}_dc"][:, 0]
    assert dc[0] > 29000 and dc[1] > 29000 and dc[2] < -24000 and dc[3] < -29000 and (dc[8:] < -13000).all()
    assert (sum(c["delta_trunc"] for c in counts) > 0) == (run in DELTA_TRUNC_RUNS), run
    # the blend's integer leaves int16 only in the backward blend of the non-causal run (a deviation)
    assert (sum(c["blend_wrap"] for c in counts) > 0) == nc, run


@needs_ref
def test_tie_run_reaches_its_aim():
    """Each stream of set T takes exactly one floor(.5 + dc_mem) on a tie that rint would round the other way; no
    other run of the fixture meets one."""
    _, counts = computed("t_causal_dc_2")
    assert [c["dc_tie"] for c in counts] == [1, 1, 1]
    fx = CE.fixture()
    assert fx["tie_pcm"][:, 0, 0].tolist() == [1500, 3500, 5500] and [.003 * v for v in (1500, 3500, 5500)] == [4.5, 10.5, 16.5]
    for run in ("d_causal_dc_0", "e_causal_dc_2"):
        assert not any(c["dc_tie"] for c in computed(run)[1]), run


@needs_ref
def test_fec_rows_reach_the_synthesis_and_the_state():
    """Set F: every queued row kind is fetched into st->features (the final
    features of the streams differ), and the non-finite rows leave NaN where
    the reference leaves it."""
    out, counts = computed("f_codec_2")
    fx = CE.fixture()
    assert (fx["f_codec_2_ctrl"][:, CR.CTRL.index("fec_read_pos")] > 0).all()
    # the row of nan_row that the last lost ticks synthesise from leaves NaN in the final state; -inf ends at the clamp
    assert np.isnan(fx["f_codec_2_gru_a"][3]).all() and np.isnan(fx["f_codec_2_features"][3]).sum() == 1
    assert fx["f_codec_2_features"][5, 0] == -10
    names = [n for n, _ in CE.F_CASES]
    nan = {n: bool(np.isnan(out["gru_a"][i]).any() or np.isnan(out["features"][i]).any()) for i, n in enumerate(names)}
    assert not any(nan[n] for n in names if n not in CE.F_NONFINITE), nan
    assert len({out["pcm"][i].tobytes() for i in range(len(names))}) == len(names), "the rows do not reach the synthesis"


def test_counters_do_not_move_the_stub():
    """The counters sit beside the control flow: a stub run counts the ring and the moves and nothing numeric."""
    ref = CR.ConcealRef(None, CR.CAUSAL | CR.DC_FILTER, 4, stub=True)
    for lost in (1, 0, 0):
        ref.tick(np.zeros(160, np.int16), bool(lost))
    assert ref.count["move_max"] == 720 and ref.count["restore_at_delay"] == 1 and ref.count["blend_wrap"] == 0
    assert ref.count["dc_tie"] == 0
