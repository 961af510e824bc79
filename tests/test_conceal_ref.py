"""The CPU reference of the PLC's state machine (tests/conceal_ref.py) against
the committed fixture tests/golden/conceal.npz, and what the reference's text
says a received frame comes back as.  The recomputation needs the
reference's compiled kernels (oracle/_ref) and is skipped without them, as in
tests/test_features_ref.py; everything else reads the fixture alone."""
import os

import numpy as np
import pytest

import conceal_ref as CR
import enc_ref

needs_ref = pytest.mark.skipif(not enc_ref.have_ref(), reason="oracle/_ref (the reference's compiled kernels) not built")


def test_fixture_shape():
    fx = CR.fixture()
    assert os.path.getsize(CR.GOLDEN) < (1 << 20)
    assert fx["pcm_in"].shape == (6, CR.NTICKS, 160) and fx["pcm_in"].dtype == np.int16
    assert np.array_equal(fx["lost"], CR.lost_matrix())
    assert np.array_equal(fx["pcm_in"], CR.received_pcm())
    for run, _, delay in CR.RUNS:
        assert fx[f"{run}_pcm"].shape == (6, CR.NTICKS, 160) and fx[f"{run}_pcm"].dtype == np.int16
        assert fx[f"{run}_buf"].shape == (6, CR.plc_buf_size(delay) + 160)
        assert fx[f"{run}_ctrl"].shape == (6, len(CR.CTRL)) and fx[f"{run}_dc"].dtype == np.float64
        assert np.isfinite(fx[f"{run}_features"]).all()
        # a concealed frame is synthesised, not silence, once a frame has been seen
        assert fx[f"{run}_pcm"][1, 4].any()
    # a loss before any frame (script 4): the loop's three teacher-forced frames are silent synthesis
    # (frame_count <= FEATURES_DELAY, lpcnet.c:239-243) but bring frame_count to 3: the tick's own output is not
    assert fx["causal_pcm"][4, 0].any()


@needs_ref
@pytest.mark.parametrize("run,options,delay", CR.RUNS, ids=[r[0] for r in CR.RUNS])
def test_fixture_equals_recomputation(run, options, delay):
    fx = CR.fixture()
    for k, v in CR.compute_run(run, options, delay).items():
        want = fx[f"{run}_{k}"]
        assert v.dtype == want.dtype and v.shape == want.shape, k
        assert np.array_equal(v.view(np.uint8), want.view(np.uint8)), (run, k)


@needs_ref
def test_compaction_scenario_equals_recomputation():
    fx = CR.fixture()
    for k, v in CR.compute_compaction().items():
        assert np.array_equal(v.view(np.uint8), fx[f"compact_{k}"].view(np.uint8)), k
    c = dict(zip(CR.CTRL, fx["compact_ctrl"]))
    assert c["fec_fill_pos"] < 100 and c["fec_keep_pos"] > 0 and c["loss_count"] == 0  # compacted; every loss had a frame


def test_received_frames_come_back_unchanged():
    """CODEC without the DC filter never writes pcm in update (lpcnet_plc.c:
    215-241 takes the else branch); CAUSAL writes it only in the blend after a
    loss (:225-229).  With the DC filter and no loss, -= lp then += lp is the
    identity modulo 2^16 (:202, :285)."""
    fx = CR.fixture()
    lost = fx["lost"].astype(bool)
    assert np.array_equal(fx["codec_pcm"][~lost], fx["pcm_in"][~lost])
    for run in ("causal", "causal_dc", "causal_d0", "causal_plc"):
        assert np.array_equal(fx[f"{run}_pcm"][0], fx["pcm_in"][0]), run  # script 0 has no loss
        for s in range(1, 6):
            blended = np.zeros(CR.NTICKS, bool)
            blended[1:] = lost[s, :-1] & ~lost[s, 1:]  # the first received frame after a loss
            same = (fx[f"{run}_pcm"][s] == fx["pcm_in"][s]).all(-1)
            assert same[~lost[s] & ~blended].all(), (run, s)
            # a blend changes the first half frame only
            assert np.array_equal(fx[f"{run}_pcm"][s][blended][:, 80:], fx["pcm_in"][s][blended][:, 80:]), (run, s)
    assert not np.array_equal(fx["causal_pcm"][1, 5, :80], fx["pcm_in"][1, 5, :80])


def test_dc_filter_follows_the_signal():
    """dc_mem is a one-pole low-pass of the received PCM (:201): after 28
    received frames of a zero-mean signal it stays small, and syn_dc is zero
    whenever the last tick was a received one (:198)."""
    fx = CR.fixture()
    ends_lost = fx["lost"][:, -1].astype(bool)
    assert ends_lost.tolist() == [False] * 5 + [True]
    assert (fx["causal_dc_dc"][~ends_lost, 1] == 0).all() and (fx["causal_dc_dc"][ends_lost, 1] != 0).all()
    assert (np.abs(fx["causal_dc_dc"][:, 0]) < 2000).all() and fx["causal_dc_dc"][:, 0].all()
    assert not fx["causal_dc"].any()  # without the filter both stay zero
