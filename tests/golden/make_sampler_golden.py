#!/usr/bin/env python3
"""Generates tests/golden/sampler_edge.npz: the cases of tests/sampler_cases.py
(tail states, edited models, non-finite conditioning) through the CPU oracle's
14-frame run (sampler_cases.oracle_run), on the port kernels.

Per (model, case) and frame: the PCM, the tail after the frame (last_sig,
deemph_mem, last_exc, the kiss99 words), the SHA-256 of both GRU states, the
number of NaN logits, of clamped samples of either sign and of threshold
ties per tree level.  Where oracle/_ref
is built the run is repeated on the reference's own compiled kernels and must
agree; the file is the same either way.  The archive is written with fixed
member timestamps, so a re-run reproduces it byte for byte.

Usage: python3 tests/golden/make_sampler_golden.py [output.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import oracle_lib as O  # noqa: E402
import sampler_cases as SC  # noqa: E402
from make_cond_golden import save  # noqa: E402


def arrays() -> dict:
    out = {k: [] for k in SC.FIXTURE_KEYS}
    for key, case in SC.RUNS:
        r = SC.oracle_run(key, case)
        if O.have_ref():
            q = SC.oracle_run(key, case, O.ref_kernels())
            for k in SC.FIXTURE_KEYS:
                assert np.array_equal(r[k], q[k]), ("port kernels differ from the reference's", key, case, k)
        for k in SC.FIXTURE_KEYS:
            out[k].append(r[k])
    a = {k: np.stack(v) for k, v in out.items()}
    a["nan_logits"] = a["nan_logits"].astype(np.int16)
    a["clamped"] = a["clamped"].astype(np.int16)
    a["ties"] = a["ties"].astype(np.int16)
    a["runs"] = np.array(SC.RUNS)
    return a


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else SC.GOLDEN
    a = arrays()
    save(path, a)
    print("wrote %s: %d runs, %d bytes (%s the reference's kernels)"
          % (path, len(SC.RUNS), os.path.getsize(path), "checked against" if O.have_ref() else "without"))


if __name__ == "__main__":
    main()
