#!/usr/bin/env python3
"""Generates tests/golden/conceal.npz (run where oracle/_ref is built).

The concealment machine's fixture, computed by tests/conceal_ref.py
(ConcealRef: the glue of lpcnet_plc.c restated line by line over the
checkers of the synthesis, the analysis, the Burg analysis and the
predictor): six streams, each with its own signal of tests/feat_signals.py
and its own script of 28 lost / received ticks (conceal_ref.SCRIPTS; the last
one with FEC adds, a NULL add and a clear), in every run of conceal_ref.RUNS
(causal, codec, causal with the DC filter, causal at FEATURES_DELAY 0, causal
on the predictor's default shape).  Per run: the PCM of every tick and, after
the last one, the control fields, st->features, st->pcm, dc_mem / syn_dc, the
synthesis GRU states and frame_count, the predictor's state and the analysis
state of every stream.  Also the FEC compaction scenario
(conceal_ref.compute_compaction).

Every received frame is checked against Burg's contract before it is used
(DC-removed where the filter is on); a frame outside it stops the maker.

Usage: python3 tests/golden/make_conceal_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import conceal_ref as CR  # noqa: E402
import enc_ref  # noqa: E402


def main():
    assert enc_ref.have_ref(), "oracle/_ref/libref_kernels.so missing: run `make -C oracle` with the reference tree present"
    arrays = {"pcm_in": CR.received_pcm(), "lost": CR.lost_matrix(),
              "fec_events": np.stack([CR.fec_events(s) for s in range(len(CR.SCRIPTS))])}
    for run, options, delay in CR.RUNS:
        for k, v in CR.compute_run(run, options, delay).items():
            arrays[f"{run}_{k}"] = v
        lost = arrays["lost"].astype(bool)
        print("  %-10s concealed PCM |max| %d, received rows changed %d" % (
            run, np.abs(arrays[f"{run}_pcm"][lost].astype(np.int32)).max(),
            int((arrays[f"{run}_pcm"][~lost] != arrays["pcm_in"][~lost]).any(-1).sum())))
    for k, v in CR.compute_compaction().items():
        arrays[f"compact_{k}"] = v
    np.savez_compressed(CR.GOLDEN, **arrays)
    print("wrote %s: %d arrays, %d bytes" % (CR.GOLDEN, len(arrays), os.path.getsize(CR.GOLDEN)))


if __name__ == "__main__":
    main()
