"""The tables beside the synthesis model, digest by digest (host only).

lpcnet_mi355x_side_digest returns one FNV-1a-64 per device table of the PLC
predictor (the re-tiled matrix-core A tiles and their seeds among them), one
each for the lpc_from_cepstrum and the feature extractor's constant tables,
and the PLC dims (include/lpcnet_mi355x.h gives the order).
tests/golden/side_digests.json holds them as the commit before those tables
moved out of engine.cpp into side_tables.cpp computed them: the move must not
change a byte.  A change that alters a table layout on purpose regenerates
the fixture with

    python tests/test_side_tables.py tests/golden/side_digests.json

and says so.
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "side_digests.json")
ENTRIES = 16
# name -> synthetic_model keywords
BLOBS = {"plc": dict(plc=True), "plc_small": dict(plc_small=True), "codebooks_plc": dict(codebooks=True, plc=True),
         "no_plc": dict()}
DIMS = {"plc": [57, 128, 256, 256], "plc_small": [57, 64, 128, 64], "codebooks_plc": [57, 128, 256, 256],
        "no_plc": [0, 0, 0, 0]}


def all_digests(L):
    return {name: ["%016x" % v for v in L.side_digest(L.synthetic_model(1, L.VARIANT_INT8, **kw))]
            for name, kw in BLOBS.items()}


@pytest.fixture(scope="module")
def computed():
    import lpcnet_amd as L
    return all_digests(L)


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_the_cases(golden):
    assert set(golden) == set(BLOBS)
    assert all(len(v) == ENTRIES for v in golden.values())
    for name, v in golden.items():
        d = [int(x, 16) for x in v]
        assert d[12:] == DIMS[name], name
        # ten PLC tables exactly when the blob carries the records; the constant tables always
        assert all((x != 0) == (name != "no_plc") for x in d[:10]), name
        assert d[10] != 0 and d[11] != 0
    # the constant tables do not depend on the blob; the codebooks leave the PLC tables alone
    assert len({tuple(v[10:12]) for v in golden.values()}) == 1
    assert golden["codebooks_plc"] == golden["plc"]
    assert golden["plc_small"][:10] != golden["plc"][:10]


@pytest.mark.parametrize("name", sorted(BLOBS))
def test_tables_match_the_parent(computed, golden, name):
    diff = [i for i in range(ENTRIES) if computed[name][i] != golden[name][i]]
    assert not diff, "%s: entries %s differ from the fixture" % (name, diff)


def test_no_blob_and_bad_arguments(golden):
    import ctypes as C
    import lpcnet_amd as L
    # no blob at all: the constant tables only
    none = ["%016x" % v for v in L.side_digest(None)]
    assert none == golden["no_plc"]
    # a blob that is not one, an fp32 blob with PLC records: no usable PLC records
    assert ["%016x" % v for v in L.side_digest(b"not a blob")] == golden["no_plc"]
    fp32 = L.synthetic_model(1, L.VARIANT_FP32, plc=True)
    assert ["%016x" % v for v in L.side_digest(fp32)] == golden["no_plc"]
    out = (C.c_uint64 * ENTRIES)()
    assert L.lib.lpcnet_mi355x_side_digest(None, 0, out, ENTRIES - 1) == -1
    assert L.last_error() == "bad arguments"
    assert L.lib.lpcnet_mi355x_side_digest(None, 0, None, ENTRIES) == -1


if __name__ == "__main__":
    sys.path.insert(0, os.environ.get("LPCNET_TREE", os.path.dirname(HERE)))
    import lpcnet_amd
    with open(sys.argv[1], "w") as out:
        json.dump(all_digests(lpcnet_amd), out, indent=0, sort_keys=True)
        out.write("\n")
