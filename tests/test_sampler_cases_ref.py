"""The sampler edge cases of tests/sampler_cases.py on the CPU oracle: the
fixture tests/golden/sampler_edge.npz is what the port kernels, the -O3 AVX2
build of the restatement and the reference's own compiled kernels compute,
the maker reproduces it byte for byte, and every case is what its name says
(the membership conditions below: conditions of the case, not measurements).

A maintainer's check (run on scratch copies of oracle/lpcnet_oracle.c, not
kept as code): each of these one-line mutations of the oracle makes
test_port_oracle_reproduces_the_fixture fail.  Runs of the 87 that caught it,
how many of those show no PCM difference at all (the tail or the GRU states
alone caught it), and cases that did:

  mutation                                    runs  no PCM diff  e.g.
  `<=` for `<` in the threshold compare          2       0       fc_tie alone (int8 and fp32)
  thresholds' bytes 1 and 2 swapped             79       0       every run with a finite walk
  clamp at +-32768                              79       0       fc_hi, fc_lo, sig_1e30, de_inf (PCM only)
  deemph_mem stored after the clamp             76       5       sig_1e30, sig_3e38, de_3e38
  last_sig clamped to +-32767                   79      11       sig_1e6, sig_edge, fc_lo
  rint for floor(.5 + x)                        11       0       de_m3e38, fc_factor (PCM only: ties at .5)
  FMA in pred                                   87      75       every run in last_sig; 12 in PCM
  FMA in the de-emphasis                        82      63       every finite run in deemph_mem; 19 in PCM
  tanh saturating instead of NaN above 1e15      8       0       fc_ramp, cond:inf_c0, cond:inf_pitch
  teacher-forced exc as o - (pd + pred)          0       -       not separated: dropped

The last one regroups a float sum whose result passes through the u-law
quantiser.  It changed no excitation in the 237 teacher-forced samples of any
run, nor over 300 further teacher seeds of 10 fully teacher-forced frames each
(normal teachers of sigma 30 to 32767) on the plain int8 model, so no teacher
of that size separates it and it is not a case here."""
import filecmp
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as O
import sampler_cases as SC

HERE = os.path.dirname(os.path.abspath(__file__))
_runs = {}


def runs(which: str) -> dict:
    """{(model key, case): oracle_run} of every run on 'port', 'avx2' or 'ref' kernels, computed once"""
    if which not in _runs:
        kw = {"port": {}, "avx2": {"avx2_build": True}, "ref": {"kernels": O.ref_kernels()}}[which]
        with ThreadPoolExecutor(8) as ex:  # ctypes calls release the GIL
            _runs[which] = dict(zip(SC.RUNS, ex.map(lambda r: SC.oracle_run(r[0], r[1], **kw), SC.RUNS)))
    return _runs[which]


def fixture_errors(got: dict) -> list:
    err = []
    for (key, case), r in got.items():
        exp = SC.expected(key, case)
        tag = "%s %s" % (key, case)
        for f in range(SC.NFRAMES):
            d = np.flatnonzero(r["pcm"][f] != exp["pcm"][f])
            if d.size:
                err.append("%s frame %d: pcm differs from the fixture at %d samples, first %s" % (tag, f, d.size, d[:6].tolist()))
            err += SC.tail_diff(tag, f, r["tail"][f], exp["tail"][f], "fixture")
            if not np.array_equal(r["digest"][f], exp["digest"][f]):
                err.append("%s frame %d: the GRU states' digest differs from the fixture's" % (tag, f))
            for k in ("nan_logits", "clamped", "ties"):
                if not np.array_equal(r[k][f], exp[k][f]):
                    err.append("%s frame %d: %s %s, the fixture has %s" % (tag, f, k, r[k][f].tolist(), exp[k][f].tolist()))
    return err


def report(err: list):
    assert not err, "%d mismatches; the first: %s" % (len(err), "\n".join(err[:8]))


def test_fixture_lists_every_run():
    fx = SC.fixture()
    assert [tuple(r) for r in fx["runs"].tolist()] == SC.RUNS
    assert fx["pcm"].shape == (len(SC.RUNS), SC.NFRAMES, SC.FRAME) and fx["tail"].shape == (len(SC.RUNS), SC.NFRAMES, SC.TAIL_WORDS)
    assert os.path.getsize(SC.GOLDEN) <= os.path.getsize(os.path.join(O.GOLDEN, "cond_edge.npz"))


def test_port_oracle_reproduces_the_fixture():
    report(fixture_errors(runs("port")))


@pytest.mark.skipif(not O.have_avx2_build(), reason="oracle/liblpcnet_oracle_avx2.so not built")
def test_avx2_build_reproduces_the_fixture():
    report(fixture_errors(runs("avx2")))


@pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built (no reference tree)")
def test_reference_kernels_reproduce_the_fixture():
    report(fixture_errors(runs("ref")))


def test_maker_is_byte_reproducible(tmp_path):
    out = str(tmp_path / "sampler_edge.npz")
    subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_sampler_golden.py"), out], check=True, capture_output=True,
                   env=dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE])))
    assert filecmp.cmp(out, SC.GOLDEN, shallow=False)


def test_logit_table_is_the_oracles():
    """LT is the table the oracle walks with: on fc_tie every traced logit is one of its entries, bit for bit"""
    lg = traced(runs("port")[("fc_tie/int8", "plain")])
    assert np.isin(lg.view(np.uint32), SC.LT.view(np.uint32)).all()


# -- membership conditions ----------------------------------------------------------------------------

OLD_FC_LIMIT = 2.0 ** 59   # the bound the engine held the dual-FC nodes to before the select-free tanh's true domain
TANH_FIN_BOUND = 2.0 ** 30  # device_math.h kTanhFinBound


def traced(r) -> np.ndarray:
    """the logits of the samples that ran: [samples, 8]"""
    return np.concatenate([r["logits"][f, :SC.SCHEDULE[f][0]] for f in range(2, SC.NFRAMES)])


@pytest.mark.parametrize("var", list(SC.VARIANTS))
def test_edited_models_are_what_they_claim(var):
    R = {e: runs("port")[("%s/%s" % (e, var), "plain")] for e in SC.EDITED}
    ties = R["fc_tie"]["ties"].sum(0)
    assert ties.sum() >= 20 and (ties >= 1).all(), ties
    lg = traced(R["fc_mid"])
    assert TANH_FIN_BOUND < SC.node_bound("fc_mid/" + var) < OLD_FC_LIMIT
    assert np.isnan(lg).sum() >= 1000 and np.isfinite(lg).sum() >= 1000
    lg = traced(R["fc_ramp"])
    assert SC.node_bound("fc_ramp/" + var) > OLD_FC_LIMIT
    assert np.isnan(lg).any() and np.isfinite(lg).any()
    lg = traced(R["fc_factor"])
    assert np.isnan(lg).any() and (lg == np.inf).any() and (lg == -np.inf).any()
    hi, lo = R["fc_hi"]["clamped"].sum(0), R["fc_lo"]["clamped"].sum(0)
    assert hi[0] >= 1000 and hi[1] == 0 and lo[1] >= 1000 and lo[0] == 0, (hi, lo)
    for f in range(2, SC.NFRAMES):  # the excitation is 255 / 0 wherever the network chose it
        n, pre = SC.SCHEDULE[f]
        assert (R["fc_hi"]["exc"][f, pre:n] == 255).all() and (R["fc_lo"]["exc"][f, pre:n] == 0).all()
    gb = R["gb_sat"]["gru_b"].view(np.float32)
    assert (gb == 1).any() and (gb == -1).any()
    for e in ("gb_in_over", "gb_both_over", "ga_zrbias"):  # the edit is felt: the plain model gives other PCM on the same frames
        o = O.Oracle(SC.model(var), SC.VARIANTS[var])
        plain = np.stack([o.synthesize(f) for f in SC.features("%s/%s" % (e, var), "plain")[:5]])
        assert not np.array_equal(R[e]["pcm"][2:5], plain[2:5]), e
    ga = R["ga_hbias"]["gru_a"].view(np.float32)[-1]
    gn = R["gb_nonfinite"]
    if var == "int8":
        assert np.flatnonzero(np.isnan(ga)).tolist() == [5, 100, 300] and ga[200] == 1.0
        assert gn["nan_logits"].sum() == 0 and not np.isnan(gn["gru_b"].view(np.float32)).any()
    else:
        assert np.isnan(ga).all()
        assert np.isnan(gn["gru_b"].view(np.float32)[-1]).any() and gn["nan_logits"].sum() > 0
        assert max(gn["pcm"][f].max() for f in range(SC.NFRAMES) if SC.SCHEDULE[f][1] == 0) <= 0


@pytest.mark.parametrize("var", list(SC.VARIANTS))
def test_tails_are_what_they_claim(var):
    R = {t: runs("port")[(var, t)] for t in SC.TAILS}
    for t in SC.RECOVERING:
        c = R[t]["clamped"].sum(1)
        assert c[SC.TAIL_AFTER + 1:].sum() > 0 or t in ("sig_denorm",), t   # the state reaches the clamp ...
        assert c[-4:].sum() == 0 and np.abs(R[t]["pcm"][-4:].astype(np.int32)).max() < 32767, t  # ... and the run leaves it
    f = SC.TAIL_AFTER + 1  # until the teacher of frame 5 turns inf into inf - inf
    assert (R["de_inf"]["pcm"][f] == 32767).all() and not R["de_nan"]["pcm"][f].any()
    assert not R["de_nan"]["pcm"][-4:].any()
    assert R["gb_nan"]["nan_logits"][SC.TAIL_AFTER + 1:].sum() > 0
    for t in SC.TAILS:  # what was written is what the record of frame 3 holds
        w = R[t]["tail"][SC.TAIL_AFTER]
        assert w[17] == SC.LAST_EXC
    assert (R["rng_zero"]["tail"][SC.TAIL_AFTER][18:] == 0).all() and (R["rng_ones"]["tail"][SC.TAIL_AFTER][18:] == 0xFFFFFFFF).all()
    assert np.array_equal(R["sig_edge"]["tail"][SC.TAIL_AFTER][:16].view(np.float32), np.array(SC.EDGE8 + SC.EDGE8, np.float32))


@pytest.mark.parametrize("var", list(SC.VARIANTS))
def test_conditioning_cases_reach_synthesis(var):
    """the non-finite class leaves a NaN GRU_A state behind in most sequences, and lpc_wide clamps"""
    R = {s: runs("port")[(var, "cond:" + s)] for s in SC.NONFINITE}
    nan_state = [s for s in SC.NONFINITE if np.isnan(R[s]["gru_a"].view(np.float32)).any()]
    assert {"pitch_huge", "nan_band", "inf_c0", "inf_pitch", "max_float"} <= set(nan_state), nan_state
    assert R["lpc_wide"]["clamped"].sum() >= 500
