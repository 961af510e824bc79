"""The CPU reference of the PLC's non-causal mode (tests/conceal_nc_ref.py)
against the committed fixture tests/golden/conceal_noncausal.npz, and what
the reference's text alone says an all-received script comes back as.  The
recomputation needs the reference's compiled kernels (oracle/_ref) and is
skipped without them, as in tests/test_conceal_ref.py; the rest reads the
fixture alone."""
import os

import numpy as np
import pytest

import conceal_nc_ref as NR
import conceal_ref as CR
import enc_ref

needs_ref = pytest.mark.skipif(not enc_ref.have_ref(), reason="oracle/_ref (the reference's compiled kernels) not built")


def delayed(pcm_in):
    """lpcnet_plc.c:440-448 on a script without a loss: tick t gives
    in[t-1][80:] then in[t][:80], zeros standing in for in[-1].  With the DC
    filter, pcm[i] - lp[i] comes back as + lp[i] half a frame later through
    dc_buf, the identity modulo 2^16."""
    want = np.zeros_like(pcm_in)
    want[:, :80] = np.concatenate([np.zeros((1, 80), np.int16), pcm_in[:-1, 80:]])
    want[:, 80:] = pcm_in[:, :80]
    return want


def test_fixture_shape():
    fx = NR.fixture()
    assert os.path.getsize(NR.GOLDEN) < os.path.getsize(CR.GOLDEN)
    assert np.array_equal(fx["lost"], CR.lost_matrix())
    for run, _ in NR.RUNS:
        assert fx[f"{run}_pcm"].shape == (6, CR.NTICKS, 160) and fx[f"{run}_pcm"].dtype == np.int16
        assert fx[f"{run}_pcm_in"].shape == (6, CR.NTICKS, 160) and len(fx[f"{run}_signals"]) == 6
        for s, name in enumerate(fx[f"{run}_signals"]):
            assert np.array_equal(fx[f"{run}_pcm_in"][s], NR.signal_pcm(str(name))), (run, s)
        assert fx[f"{run}_buf"].shape == (6, 160) and fx[f"{run}_queued_samples"].shape == (6, 160)
        assert fx[f"{run}_dcbuf"].shape == (6, 80) and fx[f"{run}_dc"].dtype == np.float64
        assert fx[f"{run}_ctrl"].shape == (6, len(CR.CTRL)) and np.isfinite(fx[f"{run}_features"]).all()
        # script 5 ends on a lost tick, script 3 on a received one straight after a loss: its update is still queued
        assert fx[f"{run}_queued_update"].tolist() == [0, 0, 0, 1, 0, 0]
        assert fx[f"{run}_queued_samples"][3].any()
        assert fx[f"{run}_pcm"][1, 4].any(), "a concealed frame is synthesised, not silence"
    # the streams kept their own signals: no frame left Burg's contract under either run
    assert [str(n) for n in fx["noncausal_signals"]] == CR.SIGNALS
    assert not fx["noncausal_dcbuf"].any() and not fx["noncausal_dc"].any()  # without the filter they stay zero
    assert fx["noncausal_dc_dcbuf"].any() and fx["noncausal_dc_dc"][:, 0].all()


def test_delay_identity_in_the_fixture():
    fx = NR.fixture()
    lost = fx["lost"].astype(bool)
    for run, _ in NR.RUNS:
        assert not lost[0].any()
        assert np.array_equal(fx[f"{run}_pcm"][0], delayed(fx[f"{run}_pcm_in"][0])), run
        # any received tick whose predecessor was received too gives back the delayed signal
        for s in range(1, 6):
            both = np.zeros(CR.NTICKS, bool)
            both[1:] = ~lost[s, 1:] & ~lost[s, :-1]
            assert np.array_equal(fx[f"{run}_pcm"][s][both], delayed(fx[f"{run}_pcm_in"][s])[both]), (run, s)


@needs_ref
@pytest.mark.parametrize("run,options", NR.RUNS, ids=[r[0] for r in NR.RUNS])
@pytest.mark.parametrize("stream", [2, 5])
def test_fixture_equals_recomputation(run, options, stream):
    """One stream of each run: script 2 (losses back to back, the queue consumed
    by a conceal) and script 5 (FEC events, ends on a lost tick)."""
    fx = NR.fixture()
    got = NR.compute_run(options, fx[f"{run}_pcm_in"], streams=[stream])
    for k, v in got.items():
        want = fx[f"{run}_{k}"][stream:stream + 1]
        assert v.dtype == want.dtype and v.shape == want.shape, k
        assert np.array_equal(v.view(np.uint8), want.view(np.uint8)), (run, k)


@needs_ref
@pytest.mark.parametrize("options", [CR.NONCAUSAL, CR.NONCAUSAL | CR.DC_FILTER], ids=["plain", "dc"])
def test_delay_identity_of_the_restatement(options):
    """On an all-received script the output is the input delayed by
    TRAINING_OFFSET: this follows from :440-448 alone, whatever the networks compute."""
    pcm_in = CR.received_pcm()[1]  # another signal than the fixture's script 0
    ref = NR.ConcealNcRef(NR.model_blob(), options)
    out = np.stack([ref.tick(pcm_in[t], False) for t in range(8)])
    assert np.array_equal(out, delayed(pcm_in[:8]))
    assert ref.queued_update == 0 and ref.loss_count == 0
