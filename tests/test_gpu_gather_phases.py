"""mf_kernel<4>'s gathers in two places: the six GRU_A waves issue the r and
the z rows behind barrier X (waves 4/5 their r rows at raised priority) and
the h rows from inside the staged elementwise step, behind the r stage's
front half, with the waits' counts moved accordingly.  Such a change can let
a wave issue with stale index words or offsets, wait for the wrong rows, or
go wrong in a ragged workgroup; a hand-off between the waves (the variants
this round measured used more workgroup barriers) can also break the barrier
parity of some path, which shows as a hang at the step's time limit.  So
EVERY stream is compared with the independent lockstep kernel
(set_kernel(1)) on an identical batch, bit for bit: the PCM of all streams
and the final GRU_A state of all streams.

1026 streams = 257 workgroups of four, the last with two streams (1024 is the
smallest batch that selects four streams per workgroup).  Synthetic streams
are silent for their first two frames, so a case runs 4 frames (5 in one
device-resident call in case 2; 3 + 3 around the resets of case 5).

Case 5: LPCNetBatch.reset(stream) restarts a stream's FEATURES_DELAY count,
so resetting all four streams of a workgroup makes that workgroup inactive
for two frames (it returns before the sample loop) beside active ones."""
import numpy as np
import pytest

import lpcnet_amd as L

pytestmark = pytest.mark.gpu

B = 1026
F = 4        # frames compared per case
F_LONG = 5   # the device-resident call of case 2
F_RESET = 3  # case 5: frames before and after the resets
# case 5: whole workgroups (0, 2, 3, 255 and the ragged 256) and one stream of workgroup 100
RESET = [0, 1, 2, 3, 8, 9, 10, 11, 12, 13, 14, 15, 402, 1020, 1021, 1022, 1023, 1024, 1025]


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def gru_a_states(b):
    return np.stack([bits(b.get_state(s)["gru_a_state"]) for s in range(b.B)])


_cache = {}


def features():
    """[2 * F_RESET][B][20], the same for every case"""
    if "f" not in _cache:
        _cache["f"] = np.ascontiguousarray(np.stack([L.synthetic_features(s, 2 * F_RESET)[:, :20] for s in range(B)], 1))
    return _cache["f"]


def lockstep():
    b = L.LPCNetBatch(B, 0, L.synthetic_model(1, L.VARIANT_INT8))
    b.set_kernel(1)
    assert b.info().quad_path not in (4, 6, 7)
    return b


def reference():
    """Lockstep kernel, per-frame calls, computed once:
    (pcm [F_LONG][B][160], GRU_A states after F frames, after F_LONG frames)"""
    if "ref" not in _cache:
        b = lockstep()
        allf = features()
        pcm = [b.synthesize(allf[f]) for f in range(F)]
        st_f = gru_a_states(b)
        pcm += [b.synthesize(allf[f]) for f in range(F, F_LONG)]
        pcm = np.stack(pcm)
        assert np.abs(pcm[2:F].astype(np.float64)).mean() > 100  # the streams are not silent
        _cache["ref"] = (pcm, st_f, gru_a_states(b))
        b.close()
    return _cache["ref"]


def run_with_resets(b):
    allf = features()
    pcm = [b.synthesize(allf[f]) for f in range(F_RESET)]
    for s in RESET:
        b.reset(s)
    pcm += [b.synthesize(allf[f]) for f in range(F_RESET, 2 * F_RESET)]
    return np.stack(pcm), gru_a_states(b)


def mf_batch(monkeypatch):
    monkeypatch.setenv("LPCNET_MFW", "0")
    b = L.LPCNetBatch(B, 0, L.synthetic_model(1, L.VARIANT_INT8))
    b.set_kernel(4)
    info = b.info()
    assert info.quad_path == 4 and info.streams_per_workgroup == 4
    return b


def same(out, ref_pcm, st, ref_st):
    bad = np.flatnonzero((out != ref_pcm).any(axis=(0, 2)))
    assert bad.size == 0, f"PCM differs in {bad.size} streams, first {bad[:8]}"
    bad = np.flatnonzero((st != ref_st).any(axis=1))
    assert bad.size == 0, f"GRU_A state differs in {bad.size} streams, first {bad[:8]}"


def check_per_frame(monkeypatch):
    ref_pcm, ref_st, _ = reference()
    b = mf_batch(monkeypatch)
    allf = features()
    out = np.stack([b.synthesize(allf[f]) for f in range(F)])
    same(out, ref_pcm[:F], gru_a_states(b), ref_st)
    return b


def test_per_frame_ragged(require_gpu, monkeypatch):
    """Case 1: per-frame calls, 257 workgroups, the last with two streams."""
    b = check_per_frame(monkeypatch)
    assert b.info().kernel_name.startswith("mf_kernel<4, 0, false")


def test_device_resident_frames(require_gpu, monkeypatch):
    """Case 2: one synthesize_frames call of 5 frames == per-frame lockstep
    calls (the frame-start barrier and the next frame's staging between the
    gathers of two frames)."""
    ref_pcm, _, ref_st = reference()
    b = mf_batch(monkeypatch)
    allf = features()[:F_LONG]
    df = b.device_alloc(allf.nbytes)
    dp = b.device_alloc(F_LONG * B * 160 * 2)
    b.h2d(df, allf)
    b.synthesize_frames(None, df, dp, F_LONG)
    b.sync()
    out = np.zeros((F_LONG, B, 160), np.int16)
    b.d2h(out, dp)
    b.device_free(df)
    b.device_free(dp)
    same(out, ref_pcm, gru_a_states(b), ref_st)


def test_forced_split(require_gpu, monkeypatch):
    """Case 3: the split instance (all 36 gathers up front, the hosted sums'
    merge behind the last of them)."""
    monkeypatch.setenv("LPCNET_MF_FORCE_SPLIT", "1")
    b = check_per_frame(monkeypatch)
    assert b.info().kernel_name.startswith("mf_kernel<4, 0, true")


def test_mixed_forms(require_gpu, monkeypatch):
    """Case 4: workgroups split between the select-free and the exact form."""
    monkeypatch.setenv("LPCNET_MF_ZR_BOUND", "0.05")
    check_per_frame(monkeypatch)


def test_inactive_workgroups_beside_active(require_gpu, monkeypatch):
    """Case 5: after three frames, five whole workgroups (the ragged one
    among them) and one stream of another are reset: for two frames those
    workgroups return before the sample loop beside 252 active ones, in the
    third they run again."""
    rb = lockstep()
    ref_pcm, ref_st = run_with_resets(rb)
    rb.close()
    keep = np.setdiff1d(np.arange(B), RESET)
    assert np.abs(ref_pcm[F_RESET:, keep].astype(np.float64)).mean() > 100  # the others play on
    assert not ref_pcm[F_RESET:F_RESET + 2, RESET].any()                    # the reset ones are silent for two frames
    assert ref_pcm[-1, RESET].any(axis=1).all()                             # and back in the third
    out, st = run_with_resets(mf_batch(monkeypatch))
    same(out, ref_pcm, st, ref_st)
