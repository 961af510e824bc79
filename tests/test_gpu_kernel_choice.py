"""The engine asks kernel_choice.cpp: what a batch on the device reports about
its sample kernel (info()) is what lpcnet_mi355x_kernel_choice -- the function
tests/test_kernel_choice.py pins on the CPU -- answers for the device's own
CU count, after a load and after each of the re-planning setters.  No kernel
is launched."""
import json

import numpy as np
import pytest

import lpcnet_amd as L
from test_kernel_choice import CHOICE_VARS, FIXTURE, PLAN, choice, fixture_row

pytestmark = pytest.mark.gpu

MODELS = {"int8": False, "int8_skewed": True}
STREAMS = [1, 129, 1025, 3072]
FIELDS = ["quad_path", "streams_per_workgroup", "lds_bytes", "mfma_ops_per_group_sample", "rcp_hw"]


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def cus(require_gpu, blobs):
    """the device's CU count, as the engine reads it"""
    return choice(L, blobs["int8"], 1, 0, 0, 0, [], [])[3]


@pytest.fixture(scope="module")
def blobs():
    return {m: L.synthetic_model(1, L.VARIANT_INT8, skewed=sk) for m, sk in MODELS.items()}


def check(b, blob, model, streams, mode, rcp, cus, env, golden):
    want = dict(zip(PLAN, choice(L, blob, streams, cus, mode, rcp, [], [])[0]))
    info = b.info()
    got = {f: int(getattr(info, f)) for f in FIELDS}
    where = (model, streams, mode, rcp, cus, env)
    assert got == {f: want[f] for f in FIELDS}, where
    row = fixture_row(golden, model, streams, mode, rcp, cus, env)
    if row is not None:
        assert got == {f: row[f] for f in FIELDS}, where
    return row is not None


@pytest.mark.parametrize("env", ["-", "MFW=0", "MF2=0"])
@pytest.mark.parametrize("model", list(MODELS))
def test_info_follows_the_choice(require_gpu, monkeypatch, golden, blobs, cus, model, env):
    for v in CHOICE_VARS + ["LPCNET_KERNEL"]:
        monkeypatch.delenv(v, raising=False)
    if env != "-":
        name, val = env.split("=")
        monkeypatch.setenv("LPCNET_" + name, val)
    tab, _ = L.host_rcp_table()
    custom = int(not np.array_equal(tab, np.repeat(L.rcp_table(), 2)))
    pinned = 0
    for streams in STREAMS:
        b = L.LPCNetBatch(streams, 0, blobs[model])
        try:
            pinned += check(b, blobs[model], model, streams, 0, 0, cus, env, golden)
            # the re-planning setters
            b.set_kernel(1)
            check(b, blobs[model], model, streams, 1, 0, cus, env, golden)
            b.set_kernel(0)
            pinned += check(b, blobs[model], model, streams, 0, 0, cus, env, golden)
            b.set_rcp_table(tab)
            check(b, blobs[model], model, streams, 0, custom, cus, env, golden)
        finally:
            b.close()
    # with the fixture's 256 CUs every load and every return to mode 0 is also a fixture row
    assert cus != 256 or pinned == 2 * len(STREAMS)
