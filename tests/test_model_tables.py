"""Every table a model load hands the device, digest by digest (host only).

lpcnet_mi355x_model_digest builds the host model of a blob -- parse, plan,
re-tile -- and returns one FNV-1a-64 per device table plus the scalar blocks
(include/lpcnet_mi355x.h gives the order).  tests/golden/model_digests.json
holds those digests as the commit before the load path was split into
model_host.cpp / mf_plan.cpp computed them (profiles/r12/README.md): the
split must not move a byte.  A change that alters the planner or a table
layout on purpose regenerates the fixture with

    python tests/test_model_tables.py tests/golden/model_digests.json

and says so.  Regenerated once since: entry 0 (the sample kernels' scalar
block) of the int8 and int8_skewed models moved when MfTables::mf_h_bound
went from 1e17 to the select-free tanh's true domain (device_math.h
kTanhFinBound less the other h-input terms); no table moved.
"""
import ctypes as C
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "model_digests.json")
ENTRIES = 60
CUS = 256
# (name, variant, saturating, skewed)
MODELS = [("int8", 0, False, False), ("int8_saturating", 0, True, False), ("int8_skewed", 0, False, True),
          ("fp32", 1, False, False), ("fp32_skewed", 1, False, True)]
# (streams, wide): the plan classes 0, 0 (two streams per workgroup), 1, 2 and 3
CLASSES = [(1, 0), (512, 0), (1024, 0), (2048, 0), (8192, 1)]
# planner and load hooks: none may leak in from the caller's environment
HOOKS = ["LPCNET_MF_ITERS", "LPCNET_MF_SIMD_W", "LPCNET_MF_HOSTED_F", "LPCNET_MF_PIECE_W", "LPCNET_MF_CAPS",
         "LPCNET_MF_FORCE_SPLIT", "LPCNET_NO_QUAD", "LPCNET_NO_MFMA", "LPCNET_NO_FPK", "LPCNET_FP_FORCE_LONG",
         "LPCNET_FC_EXACT", "LPCNET_MF_EXACT", "LPCNET_MF_ZR_BOUND", "LPCNET_NO_MFW_SPLIT", "LPCNET_RCP",
         "LPCNET_LPC_GAMMA", "LPCNET_FEATURES_DELAY", "LPCNET_END2END", "LPCNET_VERBOSE", "LPCNET_MF2", "LPCNET_MFW"]


def digests(L, blob, streams, wide):
    f = L.lib.lpcnet_mi355x_model_digest
    f.restype = C.c_int
    f.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    out = (C.c_uint64 * ENTRIES)()
    n = f(blob, len(blob), streams, CUS, wide, out, ENTRIES)
    assert n == ENTRIES, (n, L.last_error())
    return ["%016x" % v for v in out]


def all_digests(L):
    for h in HOOKS:
        os.environ.pop(h, None)
    res = {}
    for name, variant, sat, skew in MODELS:
        blob = L.synthetic_model(1, variant, saturating=sat, skewed=skew)
        for streams, wide in CLASSES:
            res["%s/%d/wide%d" % (name, streams, wide)] = digests(L, blob, streams, wide)
    return res


@pytest.fixture(scope="module")
def computed(monkeypatch_module):
    import lpcnet_amd as L
    return all_digests(L)


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    for h in HOOKS:
        mp.delenv(h, raising=False)
    yield mp
    mp.undo()


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_the_cases(golden):
    want = {"%s/%d/wide%d" % (m[0], s, w) for m in MODELS for s, w in CLASSES}
    assert set(golden) == want
    assert all(len(v) == ENTRIES for v in golden.values())
    # the int8 models carry matrix-core tables (entry 30, "mf"), except the saturating one; the fp32 ones none
    for key, v in golden.items():
        has_mf = int(v[30], 16) != 0
        assert has_mf == (key.startswith("int8") and "saturating" not in key), key
    # the skewed model's wide class carries the wide split tables (entry 33, "mfw_tab")
    assert int(golden["int8_skewed/8192/wide1"][33], 16) != 0
    assert int(golden["int8/8192/wide1"][33], 16) == 0


@pytest.mark.parametrize("model", [m[0] for m in MODELS])
def test_tables_match_the_parent(computed, golden, model):
    for streams, wide in CLASSES:
        key = "%s/%d/wide%d" % (model, streams, wide)
        diff = [i for i in range(ENTRIES) if computed[key][i] != golden[key][i]]
        assert not diff, "%s: entries %s differ from the fixture" % (key, diff)


def test_tables_decode_to_the_blob():
    """tools/model_host_check (a stand-alone program over the host-only
    objects): the register tables of every int8 model and plan class, decoded
    through their slot and row tables, give back the blob's GRU_A and GRU_B
    matrices."""
    import subprocess
    root = os.path.dirname(HERE)
    env = {k: v for k, v in os.environ.items() if k not in HOOKS}
    subprocess.run(["make", "-C", root, "tools/model_host_check"], check=True, capture_output=True, env=env)
    r = subprocess.run([os.path.join(root, "tools", "model_host_check")], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.startswith("model_host_check ok"), r.stdout


if __name__ == "__main__":
    sys.path.insert(0, os.environ.get("LPCNET_TREE", os.path.dirname(HERE)))
    import lpcnet_amd
    with open(sys.argv[1], "w") as out:
        json.dump(all_digests(lpcnet_amd), out, indent=0, sort_keys=True)
        out.write("\n")
