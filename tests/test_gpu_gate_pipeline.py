"""mf_kernel's gate-major gathers and staged GRU_A elementwise step (four
streams per workgroup): the embedding rows are loaded gate by gate and each
gate's stage runs once its own rows have arrived.  What such a reordering can
break is one lane, one stream slot or one gate, so EVERY stream is compared
with the independent lockstep kernel (set_kernel(1)) on an identical batch:
the PCM of all streams over 5 frames and the final GRU_A state of all
streams, bit for bit.  Batches with a ragged last workgroup (1026 = 256 x 4
+ 2; 513 = 256 x 2 + 1 for the two-stream instances, which keep the
stream-major form and are held to the same comparison)."""
import numpy as np
import pytest

import lpcnet_amd as L

pytestmark = pytest.mark.gpu

F = 5        # frames compared per case
F_LONG = 6   # the device-resident call of case 6


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def gru_a_states(b):
    return np.stack([bits(b.get_state(s)["gru_a_state"]) for s in range(b.B)])


_feats = {}
_refs = {}


def features(B):
    """[F_LONG][B][20], the same for every case at this batch size"""
    if B not in _feats:
        _feats[B] = np.ascontiguousarray(np.stack([L.synthetic_features(s, F_LONG)[:, :20] for s in range(B)], 1))
    return _feats[B]


def reference(B, host_rcp=False):
    """Lockstep kernel, per-frame calls, computed once per (B, table):
    (pcm [F_LONG][B][160], GRU_A states after F frames, after F_LONG frames)"""
    key = (B, host_rcp)
    if key not in _refs:
        b = L.LPCNetBatch(B, 0, L.synthetic_model(1, L.VARIANT_INT8))
        b.set_kernel(1)
        if host_rcp:
            b.set_rcp_table(L.host_rcp_table()[0])
        assert b.info().quad_path not in (4, 6, 7)
        allf = features(B)
        pcm = [b.synthesize(allf[f]) for f in range(F)]
        st_f = gru_a_states(b)
        pcm += [b.synthesize(allf[f]) for f in range(F, F_LONG)]
        pcm = np.stack(pcm)
        assert np.abs(pcm[2:F].astype(np.float64)).mean() > 100  # the streams are not silent
        _refs[key] = (pcm, st_f, gru_a_states(b))
        b.close()
    return _refs[key]


def mf_batch(B, S, monkeypatch, host_rcp=False):
    monkeypatch.setenv("LPCNET_MFW", "0")
    b = L.LPCNetBatch(B, 0, L.synthetic_model(1, L.VARIANT_INT8))
    b.set_kernel(4)
    if host_rcp:
        b.set_rcp_table(L.host_rcp_table()[0])
    info = b.info()
    assert info.quad_path == 4 and info.streams_per_workgroup == S
    return b


def check_per_frame(B, S, monkeypatch, host_rcp=False):
    ref_pcm, ref_st, _ = reference(B, host_rcp)
    b = mf_batch(B, S, monkeypatch, host_rcp)
    allf = features(B)
    out = np.stack([b.synthesize(allf[f]) for f in range(F)])
    bad = np.flatnonzero((out != ref_pcm[:F]).any(axis=(0, 2)))
    assert bad.size == 0, f"PCM differs in {bad.size} streams, first {bad[:8]}"
    st = gru_a_states(b)
    bad = np.flatnonzero((st != ref_st).any(axis=1))
    assert bad.size == 0, f"GRU_A state differs in {bad.size} streams, first {bad[:8]}"
    return b


def test_four_streams_ragged(require_gpu, monkeypatch):
    """Case 1: S = 4, 257 workgroups, the last with two streams."""
    check_per_frame(1026, 4, monkeypatch)


@pytest.mark.parametrize("env", ["LPCNET_MF_EXACT=1", "LPCNET_MF_ZR_BOUND=0.05"])
def test_exact_and_mixed_forms(require_gpu, monkeypatch, env):
    """Case 2: the exact form everywhere, then workgroups split between the
    select-free and the exact form."""
    name, _, val = env.partition("=")
    monkeypatch.setenv(name, val)
    check_per_frame(1026, 4, monkeypatch)


def test_forced_split(require_gpu, monkeypatch):
    """Case 3: the hosted partial sums merge ahead of the stages."""
    monkeypatch.setenv("LPCNET_MF_FORCE_SPLIT", "1")
    b = check_per_frame(1026, 4, monkeypatch)
    assert b.info().kernel_name.startswith("mf_kernel<4, 0, true")


def test_host_rcp_table(require_gpu, monkeypatch):
    """Case 4: this host's rcpps table on both batches (the table-only
    instances, HWR = false)."""
    b = check_per_frame(1026, 4, monkeypatch, host_rcp=True)
    assert b.info().rcp_hw == 0


def test_two_streams_ragged(require_gpu, monkeypatch):
    """Case 5: S = 2 (stream-major gathers), 257 workgroups, the last with one stream."""
    check_per_frame(513, 2, monkeypatch)


def test_device_resident_frames(require_gpu, monkeypatch):
    """Case 6: one synthesize_frames call of 6 frames == the per-frame calls
    for every stream (the next frame's staging after the last sample's
    barrier Y)."""
    B = 1026
    ref_pcm, _, ref_st = reference(B)
    b = mf_batch(B, 4, monkeypatch)
    allf = features(B)
    df = b.device_alloc(allf.nbytes)
    dp = b.device_alloc(F_LONG * B * 160 * 2)
    b.h2d(df, allf)
    b.synthesize_frames(None, df, dp, F_LONG)
    b.sync()
    out = np.zeros((F_LONG, B, 160), np.int16)
    b.d2h(out, dp)
    b.device_free(df)
    b.device_free(dp)
    bad = np.flatnonzero((out != ref_pcm).any(axis=(0, 2)))
    assert bad.size == 0, f"PCM differs in {bad.size} streams, first {bad[:8]}"
    bad = np.flatnonzero((gru_a_states(b) != ref_st).any(axis=1))
    assert bad.size == 0, f"GRU_A state differs in {bad.size} streams, first {bad[:8]}"
