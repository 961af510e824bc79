"""Active and idle streams side by side in one workgroup of the matrix-core
sample kernels, bit for bit.

A stream's first `delay` frames give zeros and leave its state alone
(lpcnet.c:265-268).  The kernels decide that per stream at launch and guard
every state store with it: the GRU_A waves' per-stream flags, the sampler
lanes' flag of their own stream, the GRU_B lanes' flag of the stream whose
unit they hold.  tests/test_gpu.py resets a stream mid-run only at 4 streams,
where each is alone in its workgroup; here two streams of a running batch are
reset -- one in the middle of a workgroup, and the last of the batch -- on
every form that puts several streams into a workgroup:

* mf_kernel at 4 and 2 streams per workgroup (1024 and 512 streams);
* mf2_kernel (LPCNET_MF2=1) at 9 streams: the second workgroup partly filled;
* mfw_kernel (LPCNET_MF2=1 LPCNET_MFW=1) at 8 streams, two groups (a split
  model without a wide split form falls to the split forms of mf_kernel /
  mf2_kernel, as in tests/test_gpu_mask_models.py), and, unsplit, three
  groups at 12 streams.

Three frames through synthesize, reset(k) of the two streams, two more
frames (the reset streams' delay frames: zero PCM, GRU states bit-identical
to the reset state, their neighbours running on), then four frames through
synthesize_frames on device buffers: the reset streams turn active with the
first of them, so the run is one multi-frame launch and the host has nothing
to split.  A second variant runs one host frame after the reset: the device
run then starts with the reset streams' second delay frame, which the host
launches alone (mixed activity), before a multi-frame launch of the other
three.  Every stream's PCM of
every frame against the same sequence on the lockstep kernel
(set_kernel(1)); PCM and final GRU states of the reset streams, a neighbour
of each in its workgroup and stream 0 against the CPU oracle, restarted at
the reset.  Tolerance 0; the kernel is asserted from info()."""
import functools

import numpy as np
import pytest

import lpcnet_amd as L
import oracle_lib as O
from test_gpu_mask_models import setenv, tf
from test_gpu_masks import _frames, bits
from test_mask_models import PLAN, blob_of

pytestmark = pytest.mark.gpu

F0, F2 = 3, 4  # frames before the reset, device frames; between them F1 host frames after the reset
DELAY = 2    # the synthetic models' FEATURES_DELAY
F = F0 + DELAY + F2
MODELS = ("at_caps", "skewed_seed2")  # an unsplit and a split plan, the latter with a wide split form
# form -> (environment, streams, the reset stream in the middle of a workgroup)
FORMS = {
    "mf4": ({}, 1024, 513),
    "mf2": ({}, 512, 257),
    "mf2_kernel": ({"LPCNET_MF2": "1"}, 9, 5),
    "mfw2": ({"LPCNET_MF2": "1", "LPCNET_MFW": "1"}, 8, 3),
    "mfw3": ({"LPCNET_MF2": "1", "LPCNET_MFW": "1", "LPCNET_MFW_G": "3"}, 12, 5),
}
CASES = [(m, f) for m in MODELS for f in FORMS if not (f == "mfw3" and PLAN[m][1])]


@functools.lru_cache(maxsize=None)
def features(B):
    return np.ascontiguousarray(np.stack([L.synthetic_features(s, F)[:, :20] for s in range(B)], 1))


@functools.lru_cache(maxsize=None)
def oracle(name, stream, reset, F1):
    """(pcm [F, 160], gru_a_state, gru_b_state) of one stream, restarted after F0 frames where reset"""
    blob = blob_of(name, 0)
    f = L.synthetic_features(stream, F)[:, :20]
    o = O.Oracle(blob, 0)
    pcm = []
    for i in range(F0 + F1 + F2):
        if reset and i == F0:
            o = O.Oracle(blob, 0)
        pcm.append(o.synthesize(f[i]))
    return (np.stack(pcm),) + tuple(o.state())


def run(name, B, resets, F1, kernel=0):
    b = L.LPCNetBatch(B, 0, blob_of(name, 0))
    if kernel:
        b.set_kernel(kernel)
    info = b.info()
    allf = features(B)
    out = [b.synthesize(allf[f]) for f in range(F0)]
    fresh = {}
    for k in resets:
        b.reset(k)
        fresh[k] = b.get_state(k)
    out += [b.synthesize(allf[f]) for f in range(F0, F0 + F1)]
    held = {k: b.get_state(k) for k in resets}
    out = np.concatenate([np.stack(out), _frames(b, allf, F0 + F1, F0 + F1 + F2)], 0)
    final = {s: b.get_state(s) for s in checked(B, resets)}
    b.close()
    return out, fresh, held, final, info


def checked(B, resets):
    """the reset streams, the other stream of each one's pair (the same
    workgroup in every form) where the batch has it, and stream 0"""
    return sorted({0} | set(resets) | {k ^ 1 for k in resets if k ^ 1 < B})


@functools.lru_cache(maxsize=None)
def lockstep(name, B, resets, F1):
    out, _, _, _, info = run(name, B, resets, F1, 1)
    assert info.kernel_name.startswith("sample_kernel<"), info.kernel_name
    return out


def expect_kernel(name, form, info):
    _, split, wide = PLAN[name]
    if form in ("mf4", "mf2"):
        assert info.kernel_name == "mf_kernel<%s, 0, %s, true>" % (form[2], tf(split)), info.kernel_name
    elif form == "mf2_kernel":
        assert info.kernel_name == "mf2_kernel<4, %s, true>" % tf(split), info.kernel_name
    elif form == "mfw2" and split and not wide:
        assert info.kernel_name in ("mf_kernel<1, 0, true, true>", "mf2_kernel<4, true, true>"), info.kernel_name
    elif form == "mfw2":
        assert info.kernel_name == "mfw_kernel<true, 2, %s>" % tf(split), info.kernel_name
    else:
        assert info.kernel_name == "mfw_kernel<true, 3, false>", info.kernel_name


@pytest.mark.parametrize("F1", [2, 1])
@pytest.mark.parametrize("name,form", CASES)
def test_reset_streams_inside_a_workgroup(require_gpu, monkeypatch, name, form, F1):
    env, B, mid = FORMS[form]
    setenv(monkeypatch, **env)
    resets = (mid, B - 1)
    out, fresh, held, final, info = run(name, B, resets, F1)
    expect_kernel(name, form, info)
    assert np.abs(out.astype(np.float64)).mean() > 100
    for k in resets:
        assert not out[F0:F0 + DELAY, k].any(), k
        for key in ("gru_a_state", "gru_b_state"):
            assert np.array_equal(bits(held[k][key]), bits(fresh[k][key])), (k, key)
        assert out[F0 + DELAY:, k].any(), k
    for s in checked(B, resets):
        pcm, a, g = oracle(name, s, s in resets, F1)
        assert np.array_equal(out[:, s], pcm), s
        assert np.array_equal(bits(final[s]["gru_a_state"]), bits(a)), s
        assert np.array_equal(bits(final[s]["gru_b_state"]), bits(g)), s
    ref = lockstep(name, B, resets, F1)
    bad = np.flatnonzero((out != ref).any((0, 2)))
    assert bad.size == 0, "streams %s differ from the lockstep kernel" % bad[:8]
