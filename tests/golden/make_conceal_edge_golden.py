#!/usr/bin/env python3
"""Generates tests/golden/conceal_edge.npz (run where oracle/_ref is built).

The concealment machine's edge-case fixture, computed by tests/conceal_edge.py
through tests/conceal_ref.py and tests/conceal_nc_ref.py (lpcnet_plc.c's glue
restated line by line over the checkers of the synthesis, the analysis, the
Burg analysis and the predictor): the run sets D (the six scripts at every
FEATURES_DELAY the other fixtures leave out, in the causal and codec modes,
with and without the DC filter), E (five edge signals, each on script 3 and
on a 20-tick burst, with the DC filter, one run non-causal) and F (script 5
in the codec mode queueing edge-case FEC rows).  Per run: the PCM of every
tick and, after the last one, the control fields, st->features, st->pcm,
dc_mem / syn_dc, the GRU_B state and frame_count of every stream, and the
GRU_A state, the predictor's state and the analysis state as SHA-256 digests
(sets D and E) or in full (set F, where they are compared NaN-aware); in the
non-causal run also queued_update, queued_samples and dc_buf.

Every received frame is checked against Burg's contract before it is used
(DC-removed where the filter is on); a frame outside it stops the maker: the
signal is to be replaced, never skipped.  Prints what each run reached
(conceal_ref.COUNTERS, summed over its streams).

Usage: python3 tests/golden/make_conceal_edge_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import conceal_edge as CE  # noqa: E402
import conceal_ref as CR  # noqa: E402
import enc_ref  # noqa: E402


def main():
    assert enc_ref.have_ref(), "oracle/_ref/libref_kernels.so missing: run `make -C oracle` with the reference tree present"
    arrays = CE.compute_inputs()
    for run, _, _ in CE.RUNS:
        out, counts = CE.compute_run(run)
        for k, v in out.items():
            arrays[f"{run}_{k}"] = v
        print("  %-17s %s" % (run, " ".join("%s=%d" % (k, max(c[k] for c in counts) if k == "move_max" else sum(c[k] for c in counts))
                                            for k in CR.COUNTERS)))
    arrays = CE.pack(arrays)
    np.savez_compressed(CE.GOLDEN, **arrays)
    print("wrote %s: %d arrays, %d bytes" % (CE.GOLDEN, len(arrays), os.path.getsize(CE.GOLDEN)))


if __name__ == "__main__":
    main()
