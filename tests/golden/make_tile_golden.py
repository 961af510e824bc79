#!/usr/bin/env python3
"""Generates tests/golden/tile_edge.json: {"model/side/case": sha256} of every
run of tests/tile_cases.py (every call's outputs and the snapshot after it,
NaNs as 0x7FC00000), computed on the reference's own compiled kernels.

Refuses to run without oracle/_ref, and on a host whose rcpps is not the
pinned Intel table (the reference's activations would not be the port's);
asserts that the port's kernels give the same digests.

Usage: python3 tests/golden/make_tile_golden.py [output.json]
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import oracle_lib as O  # noqa: E402
import tile_cases as T  # noqa: E402


def main():
    if not O.have_ref():
        sys.exit("oracle/_ref (the reference's compiled kernels) is not built")
    tab, bad = O.ref_rcp_table()
    if bad or not np.array_equal(tab, O.RCP_TABLE):
        sys.exit("this host's rcpps is not the pinned table: the reference's activations differ from the port's here")
    path = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    out = {}
    for run in T.RUNS:
        out[T.key(*run)] = d = T.reference_digest(*run, table="ref")
        assert d == T.reference_digest(*run), ("port kernels differ from the reference's", run)
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d runs, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
