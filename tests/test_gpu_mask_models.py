"""Every GRU_A kernel form on the masks of tests/mask_models.py, bit for bit.

The matrix-core kernels dispatch on what mf_plan.cpp makes of the model's
mask: mf_kernel and mf2_kernel switch over a wave's own group counts (a
runtime-count default for the counts the switch does not list, 0 among
them), their split forms over every (own, hosted) pair, mfw_kernel's default
runs the full tables and relies on zero slots.  tests/test_mask_models.py
shows on the host that each family reaches the plan it is named for; here
each family runs on each form it can take:

* mf_kernel at 1, 2 and 4 streams per workgroup (3, 512, 1024 streams: the
  smallest batches that take them, model_host.cpp choose_lockstep_lds);
* mf2_kernel (LPCNET_MF2=1) at 9 streams: the second group partly filled;
* mfw_kernel (LPCNET_MF2=1 LPCNET_MFW=1) at 8 streams, two groups -- a split
  model takes the wide split form, and where that form does not exist
  (mask_models.wide_split_exists) the batch must fall to mf2_kernel's split
  form and still match; unsplit models also with three groups at 12 streams;
* the over-full masks on the automatic kernel (lockstep, weights in global
  memory) at 3 and 300 streams;
* fp32 (fp_kernel, short and long form) at 1 and 70 streams;
* the GRU_B input masks (the matrix-core GRU_B is a dense tile built from the
  index) at 3 and 1024 streams, fp32 on the lockstep kernel at 1.

Three frames of per-stream synthetic features: two through synthesize, the
third through synthesize_frames on device buffers.  PCM and final GRU states
of streams {0, B/2, B-1} against the CPU oracle, every stream's PCM against
the same batch on the lockstep kernel (set_kernel(1)), tolerance 0; the kernel
each case ran is asserted from info(), so a silent fallback fails."""
import functools

import numpy as np
import pytest

import lpcnet_amd as L
import mask_models as M
import oracle_lib as O
from test_gpu_masks import _frames, bits
from test_mask_models import FP32_FAMILIES, PLAN, blob_of

pytestmark = pytest.mark.gpu

F = 3
MF = sorted(k for k, p in PLAN.items() if p[0])
UNSPLIT = sorted(k for k, p in PLAN.items() if p[0] and not p[1])
LOCKSTEP = sorted(k for k, p in PLAN.items() if not p[0])
ENV = ("LPCNET_MF2", "LPCNET_MFW", "LPCNET_MFW_G")
FP_LONG = {"one_block": 0, "z_one_full": 1, "dense": 1}


@functools.lru_cache(maxsize=None)
def features(B):
    return np.ascontiguousarray(np.stack([L.synthetic_features(s, F)[:, :20] for s in range(B)], 1))


@functools.lru_cache(maxsize=None)
def oracle(name, variant, stream):
    o = O.Oracle(blob_of(name, variant), variant)
    f = L.synthetic_features(stream, F)[:, :20]
    pcm = np.stack([o.synthesize(f[i]) for i in range(F)])
    return (pcm,) + tuple(o.state())


def run(name, variant, B, kernel=0):
    b = L.LPCNetBatch(B, 0, blob_of(name, variant))
    if kernel:
        b.set_kernel(kernel)
    info = b.info()
    allf = features(B)
    out = np.concatenate([np.stack([b.synthesize(allf[f]) for f in range(F - 1)]), _frames(b, allf, F - 1, F)], 0)
    states = {s: b.get_state(s) for s in (0, B // 2, B - 1)}
    b.close()
    return out, states, info


@functools.lru_cache(maxsize=None)
def lockstep(name, variant, B):
    out, _, info = run(name, variant, B, 1)
    assert info.kernel_name.startswith("sample_kernel<"), info.kernel_name
    return out


def check(name, variant, B, out, states):
    assert np.abs(out.astype(np.float64)).mean() > 100
    for s in sorted(states):
        pcm, a, g = oracle(name, variant, s)
        assert np.array_equal(out[:, s], pcm), s
        assert np.array_equal(bits(states[s]["gru_a_state"]), bits(a)), s
        assert np.array_equal(bits(states[s]["gru_b_state"]), bits(g)), s
    ref = lockstep(name, variant, B)
    bad = np.flatnonzero((out != ref).any((0, 2)))
    assert bad.size == 0, "streams %s differ from the lockstep kernel" % bad[:8]


def setenv(monkeypatch, **env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def tf(x):
    return "true" if x else "false"


@pytest.mark.parametrize("B,S", [(3, 1), (512, 2), (1024, 4)])
@pytest.mark.parametrize("name", MF)
def test_mf_kernel(require_gpu, monkeypatch, name, B, S):
    setenv(monkeypatch)
    out, states, info = run(name, 0, B)
    assert info.may_saturate == 0 and info.quad_path == 4 and info.long_rows == PLAN[name][1], (info.quad_path, info.long_rows)
    assert info.kernel_name == "mf_kernel<%d, 0, %s, true>" % (S, tf(PLAN[name][1])), info.kernel_name
    check(name, 0, B, out, states)


@pytest.mark.parametrize("name", MF)
def test_mf2_kernel(require_gpu, monkeypatch, name):
    setenv(monkeypatch, LPCNET_MF2="1")
    out, states, info = run(name, 0, 9)
    assert info.may_saturate == 0 and info.quad_path == 6 and info.long_rows == PLAN[name][1], (info.quad_path, info.long_rows)
    assert info.kernel_name == "mf2_kernel<4, %s, true>" % tf(PLAN[name][1]), info.kernel_name
    check(name, 0, 9, out, states)


@pytest.mark.parametrize("name", MF)
def test_mfw_kernel_or_its_fallback(require_gpu, monkeypatch, name):
    """two groups; a split model whose mask has no wide split form must not
    run mfw_kernel: the batch stays on the split forms of mf_kernel /
    mf2_kernel (the wide plan class's tables) and still matches"""
    setenv(monkeypatch, LPCNET_MF2="1", LPCNET_MFW="1")
    _, split, wide = PLAN[name]
    out, states, info = run(name, 0, 8)
    assert info.may_saturate == 0 and info.long_rows == split
    if split and not wide:
        assert info.quad_path in (4, 6), info.quad_path
        assert info.kernel_name in ("mf_kernel<1, 0, true, true>", "mf2_kernel<4, true, true>"), info.kernel_name
    else:
        assert info.quad_path == 7 and info.streams_per_workgroup == 8, (info.quad_path, info.streams_per_workgroup)
        assert info.kernel_name == "mfw_kernel<true, 2, %s>" % tf(split), info.kernel_name
    check(name, 0, 8, out, states)


@pytest.mark.parametrize("name", UNSPLIT)
def test_mfw_kernel_three_groups(require_gpu, monkeypatch, name):
    setenv(monkeypatch, LPCNET_MF2="1", LPCNET_MFW="1", LPCNET_MFW_G="3")
    out, states, info = run(name, 0, 12)
    assert info.quad_path == 7 and info.streams_per_workgroup == 12, (info.quad_path, info.streams_per_workgroup)
    assert info.kernel_name == "mfw_kernel<true, 3, false>", info.kernel_name
    check(name, 0, 12, out, states)


@pytest.mark.parametrize("B", [3, 300])
@pytest.mark.parametrize("name", LOCKSTEP)
def test_over_full_masks_on_the_lockstep_kernel(require_gpu, monkeypatch, name, B):
    """no split fits the register tables: the automatic kernel is the
    lockstep one (its GRU_A weight sections in global memory for the dense
    mask, 442 KB)"""
    setenv(monkeypatch)
    out, states, info = run(name, 0, B)
    assert info.may_saturate == 0 and info.quad_path in (0, 1) and info.gru_a_blocks == sum(len(r) for r in M.FAMILIES[name])
    assert info.kernel_name.startswith("sample_kernel<%d, 0, false, " % info.streams_per_workgroup), info.kernel_name
    check(name, 0, B, out, states)


@pytest.mark.parametrize("B", [1, 70])
@pytest.mark.parametrize("name", FP32_FAMILIES)
def test_fp32(require_gpu, monkeypatch, name, B):
    setenv(monkeypatch)
    out, states, info = run(name, 1, B)
    assert info.quad_path == 5 and info.long_rows == FP_LONG[name], (info.quad_path, info.long_rows)
    assert info.kernel_name == "fp_kernel<0, %s, true>" % tf(FP_LONG[name]), info.kernel_name
    check(name, 1, B, out, states)


@pytest.mark.parametrize("variant,B,S", [(0, 3, 1), (0, 1024, 4), (1, 1, 1)])
@pytest.mark.parametrize("kind", M.GRU_B_KINDS)
def test_gru_b_masks(require_gpu, monkeypatch, kind, variant, B, S):
    """int8: the matrix-core GRU_B's dense tile with the mask's holes; fp32:
    fp_kernel needs a dense GRU_B, the lockstep kernel runs the sparse one"""
    setenv(monkeypatch)
    name = "gru_b_" + kind
    out, states, info = run(name, variant, B)
    if variant == 0:
        assert info.kernel_name == "mf_kernel<%d, 0, false, true>" % S, info.kernel_name
    else:
        assert info.quad_path in (0, 1) and info.kernel_name.startswith("sample_kernel<1, 1, false, "), info.kernel_name
    check(name, variant, B, out, states)
