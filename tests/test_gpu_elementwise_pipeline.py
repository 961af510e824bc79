"""mf_kernel<4>'s pipelined GRU_A elementwise step: each gate's rcpps table
reads run under the next stage's front half (ga_elementwise_staged).  The
reordering is shared by the select-free and the exact form, both table
widths' callers and the split instances, so the instance combinations that
tests/test_gpu_gate_pipeline.py does not reach are held to the same
comparison here: EVERY stream of a 1026-stream batch (257 workgroups of four
streams, the last with two; the smallest batch that runs four streams per
workgroup) against the independent lockstep kernel (set_kernel(1)) on an
identical batch -- the PCM of all streams over 5 frames and the final GRU_A
state, bit for bit, no tolerance and no stream left out."""
import re

import numpy as np
import pytest

import lpcnet_amd as L

pytestmark = pytest.mark.gpu

B = 1026
F = 5  # frames compared per case


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def gru_a_states(b):
    return np.stack([bits(b.get_state(s)["gru_a_state"]) for s in range(b.B)])


_feats = []
_refs = {}


def features():
    """[F][B][20], the same for every case"""
    if not _feats:
        _feats.append(np.ascontiguousarray(np.stack([L.synthetic_features(s, F)[:, :20] for s in range(B)], 1)))
    return _feats[0]


def reference(host_rcp):
    """Lockstep kernel, per-frame calls, computed once per table and left
    unchanged: (pcm [F][B][160], GRU_A states after F frames).  The lockstep
    kernel reads none of the LPCNET_MF_* switches."""
    if host_rcp not in _refs:
        b = L.LPCNetBatch(B, 0, L.synthetic_model(1, L.VARIANT_INT8))
        b.set_kernel(1)
        if host_rcp:
            b.set_rcp_table(L.host_rcp_table()[0])
        assert b.info().quad_path not in (4, 6, 7)
        allf = features()
        pcm = np.stack([b.synthesize(allf[f]) for f in range(F)])
        assert np.abs(pcm[2:].astype(np.float64)).mean() > 100  # the streams are not silent
        st = gru_a_states(b)
        b.close()
        pcm.setflags(write=False)
        st.setflags(write=False)
        _refs[host_rcp] = (pcm, st)
    return _refs[host_rcp]


CASES = [
    # id, environment, host table, kernel name, rcp_hw, z/r range bound the engine must report
    ("exact_host_table", {"LPCNET_MF_EXACT": "1"}, True, "mf_kernel<4, 0, false, false>", 0, "exact"),
    ("exact_forced_split", {"LPCNET_MF_EXACT": "1", "LPCNET_MF_FORCE_SPLIT": "1"}, False,
     "mf_kernel<4, 0, true, true>", 1, "exact"),
    ("forced_split_host_table", {"LPCNET_MF_FORCE_SPLIT": "1"}, True, "mf_kernel<4, 0, true, false>", 0, "model"),
    ("mixed_forced_split", {"LPCNET_MF_ZR_BOUND": "0.05", "LPCNET_MF_FORCE_SPLIT": "1"}, False,
     "mf_kernel<4, 0, true, true>", 1, "0.05"),
]

BOUNDS = re.compile(r"GRU_A range bounds: z/r (\S+) .*, h (\S+)")


def check_bounds(err, want):
    """The form a workgroup takes is not visible in its output (both forms
    compute the same), so the case checks what selects it: the range bounds
    the engine hands the kernel (reported under LPCNET_VERBOSE).  A
    workgroup takes the select-free form only while every conditioning value
    is within them: -1 sends every workgroup to the exact form, 0.05 is the
    bound with which tests/test_gpu_gate_pipeline.py splits the workgroups
    between the two forms, and the synthetic model's own bound is 130,776."""
    found = BOUNDS.findall(err)
    assert found, "the engine did not report its GRU_A range bounds"
    for zr, h in found:
        if want == "exact":
            assert float(zr) == -1.0 and float(h) == -1.0
        elif want == "0.05":
            assert float(zr) == pytest.approx(0.05, rel=1e-6) and float(h) > 1.0
        else:
            assert float(zr) > 1000.0 and float(h) > 1.0


@pytest.mark.parametrize("env,host_rcp,kernel,rcp_hw,bounds", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_instance_matches_lockstep(require_gpu, monkeypatch, capfd, env, host_rcp, kernel, rcp_hw, bounds):
    ref_pcm, ref_st = reference(host_rcp)
    capfd.readouterr()
    monkeypatch.setenv("LPCNET_MFW", "0")
    monkeypatch.setenv("LPCNET_VERBOSE", "1")
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    b = L.LPCNetBatch(B, 0, L.synthetic_model(1, L.VARIANT_INT8))
    b.set_kernel(4)
    if host_rcp:
        b.set_rcp_table(L.host_rcp_table()[0])
    info = b.info()
    assert info.quad_path == 4 and info.streams_per_workgroup == 4
    assert info.kernel_name == kernel
    assert info.rcp_hw == rcp_hw
    allf = features()
    out = np.stack([b.synthesize(allf[f]) for f in range(F)])
    st = gru_a_states(b)
    b.close()
    check_bounds(capfd.readouterr().err, bounds)
    bad = np.flatnonzero((out != ref_pcm).any(axis=(0, 2)))
    assert bad.size == 0, f"PCM differs in {bad.size} streams, first {bad[:8]}"
    bad = np.flatnonzero((st != ref_st).any(axis=1))
    assert bad.size == 0, f"GRU_A state differs in {bad.size} streams, first {bad[:8]}"
